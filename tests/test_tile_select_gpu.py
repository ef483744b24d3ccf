"""statmc_score_tile_select and statmc_gate_tiles on the device against the numpy restatement (tests/tile_select_reference.py, whose
own cases tests/test_tile_select_cpu.py checks): every plane bit for bit -- the floats as uint32, the counts as integers -- no
tolerance anywhere.  Every tile size on films with partial tiles, one pixel, more than one workgroup; every special bit pattern,
constant images, heavy ties; the ranks together and singly; NULL planes, unaligned images, planes full of garbage between guard words,
pixels shuffled within their tiles; statmc_score_tiles, statmc_score_select and statmc_score_count_above on the same data; the gate in
and out of place, with memory over three calls, through statmc_compact_offsets and statmc_plan_samples; both entries on a library
stream behind a gate and an event; FilmStats.score_tile_quantiles / gate_tiles.  The select kernel does not stride: a workgroup takes
one group of tiles, so no film exists on which it takes two."""
import ctypes as C

import numpy as np
import pytest

import select_reference as sel_ref
import tile_select_reference as ref
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
# one pixel; two; a partial tile of every size; exactly one 8-tile; one pixel over it; rows shorter than a quad apart; exactly one
# 64-tile; one pixel over it in x, a partial one in y; more rows than columns, three tiles of 64 down; five tiles of 64 across
FILMS = [(1, 1), (2, 1), (7, 3), (8, 8), (9, 9), (17, 5), (64, 64), (65, 33), (67, 130), (257, 70)]
IMAGES = ["random_bits", "constant_normal", "constant_subnormal", "all_infinite", "all_zero", "ties"]
CONSTANTS = {"constant_normal": 0x3F400000, "constant_subnormal": 0x00000301, "all_infinite": 0x7F800000, "all_zero": 0}
SPECIAL = [0x7FC00000, 0xFFC00001, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0]
NUMS, DEN = [0, 10, 19, 20], 20      # q = 0, 1/2, 19/20, 1


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_offset(a):
    """the same values in an image that starts 4 bytes into its allocation: 4-byte but not 16-byte aligned"""
    import torch
    flat = torch.from_numpy(np.array(a, order="C").reshape(-1)).cuda()
    buf = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda:0")
    view = buf[1:1 + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(a.shape)


def from_bits(b):
    return np.asarray(b, np.uint32).view(F32)


def image(name, W, H):
    rng = np.random.default_rng(W * 1000 + H + IMAGES.index(name))
    px = W * H
    if name == "random_bits":      # every class and exponent; the special patterns put in by hand where the film has room
        b = rng.integers(0, 2 ** 32, px, dtype=np.uint64).astype(np.uint32)
        if px > 2 * len(SPECIAL):
            b[rng.choice(px, len(SPECIAL), replace=False)] = SPECIAL
        return from_bits(b).reshape(H, W)
    if name in CONSTANTS:
        return from_bits(np.full((H, W), CONSTANTS[name], np.uint32))
    if name == "ties":             # a few distinct values per tile, specials among them: n_equal > 1 at every rank of a full tile
        return from_bits(rng.choice(np.array([0x3C23D70A, 0x3CA3D70A, 0x3F800000, 0x7F800000, 0x80000000], np.uint32), (H, W)))
    raise KeyError(name)


_cases = {}


def case(film, name):
    """(score image, {tile: the restated planes of NUMS / DEN}), computed once and left unchanged"""
    if (film, name) not in _cases:
        W, H = film
        score = image(name, W, H)
        score.setflags(write=False)
        want = {}
        for tile in ref.TILES:
            w = ref.tile_select_ref(score, tile, NUMS, DEN)
            for f in w.values():
                for a in f:
                    a.setflags(write=False)
            want[tile] = w
        _cases[(film, name)] = (score, want)
    return _cases[(film, name)]


def run(gpu, d_score, tile, nums=NUMS, den=DEN, **kw):
    import torch
    res = gpu.score_tile_select(d_score, tile, nums, den, **kw)
    if "stream" not in kw:
        torch.cuda.synchronize()
    return gpu.read_tile_quantiles(res)


def assert_planes(got, want, what, slots=range(4), fields=ref.FIELDS):
    """got[f][k] is the plane of want's slot slots[k]"""
    assert sorted(got) == sorted(fields), what
    for f in fields:
        assert len(got[f]) == len(slots), (what, f)
        for k, s in enumerate(slots):
            g, w = got[f][k], want[f][s]
            assert g.shape == w.shape and g.dtype == w.dtype, (what, f, s, g.shape, g.dtype)
            g, w = (g.view(np.uint32), w.view(np.uint32)) if f == "value" else (g, w)
            if not np.array_equal(g, w):
                at = tuple(np.argwhere(g != w)[0])
                raise AssertionError("%s: %s[%d] differs; first at tile %s: %x, restated %x" % (what, f, s, at, int(g[at]), int(w[at])))


# ---------------------------------------------------------------- 1. every plane, every tile size, bit for bit
@pytest.mark.parametrize("name", IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_tile_quantiles_equal_the_restatement_bit_for_bit(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    for tile in ref.TILES:
        assert_planes(run(gpu, d_score, tile), want[tile], (film, name, tile))
    if name == "ties" and film[0] * film[1] >= 64:
        assert min(int(a.max()) for a in want[8]["n_equal"]) > 1
    if name == "all_infinite":
        assert all((a.view(np.uint32) == 0x7F800000).all() for a in want[16]["value"])      # the tile stays open under any finite threshold


@pytest.mark.parametrize("name", ["random_bits", "ties"])
@pytest.mark.parametrize("film", [(9, 9), (67, 130), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_ranks_singly_and_in_pairs_equal_the_four_together(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    for tile in ref.TILES:
        for s in range(4):
            assert_planes(run(gpu, d_score, tile, [NUMS[s]]), want[tile], (film, name, tile, s), slots=[s])
        assert_planes(run(gpu, d_score, tile, [NUMS[3], NUMS[1]]), want[tile], (film, name, tile, "pair"), slots=[3, 1])
        assert_planes(run(gpu, d_score, tile, [NUMS[2], NUMS[2], NUMS[0]]), want[tile], (film, name, tile, "repeat"), slots=[2, 2, 0])


def test_other_denominators_and_the_rank_rule_at_its_edges(gpu):
    score, _ = case((257, 70), "random_bits")
    d_score = dev(score)
    for tile in ref.TILES:
        for nums, den in (([1, 65535, 65536, 0], 65536), ([1], 1), ([0], 1), ([1, 2, 3], 3), ([1, 63, 64], 64)):
            w = ref.tile_select_ref(score, tile, nums, den)
            assert_planes(run(gpu, d_score, tile, nums, den), w, (tile, nums, den), slots=range(len(nums)))


# ---------------------------------------------------------------- 2. NULL planes, alignment, garbage, guards, shuffles
def test_null_planes_are_not_formed_and_only_the_planes_are_written(gpu):
    """each plane lies between guard words in a buffer of its own, full of garbage; the score image's bytes before and after"""
    import torch
    score, want = case((257, 70), "random_bits")
    d_score = dev(score)
    before = d_score.view(torch.int32).cpu().numpy().copy()
    guard = 64
    for tile in ref.TILES:
        ty, tx = gpu.tile_grid(70, 257, tile)
        for fields in (ref.FIELDS, ("value",), ("n_below", "n_equal"), ("n_equal",)):
            bufs, out = {}, {}
            for f in fields:
                dt = torch.float32 if f == "value" else torch.int32
                bufs[f] = [torch.full((guard + ty * tx + guard,), 7, dtype=dt, device="cuda:0") for _ in range(4)]
                out[f] = [b[guard:guard + ty * tx].view(ty, tx) for b in bufs[f]]
            assert_planes(run(gpu, d_score, tile, fields=fields, out=out), want[tile], (tile, fields), fields=fields)
            for f in fields:
                for b in bufs[f]:
                    host = b.cpu().numpy()
                    assert np.all(host[:guard] == 7) and np.all(host[guard + ty * tx:] == 7), (tile, f)
        # a plane left out within a field: slot 1's value and slot 2's counts are NULL
        out = {"value": [torch.full((ty, tx), 3.0, device="cuda:0") if s != 1 else None for s in range(4)],
               "n_below": [torch.full((ty, tx), 3, dtype=torch.int32, device="cuda:0") if s != 2 else None for s in range(4)]}
        got = run(gpu, d_score, tile, fields=("value", "n_below"), out=out)
        for s in range(4):
            assert (got["value"][s] is None) == (s == 1) and (got["n_below"][s] is None) == (s == 2)
            if s != 1:
                assert np.array_equal(got["value"][s].view(np.uint32), want[tile]["value"][s].view(np.uint32)), (tile, s)
            if s != 2:
                assert np.array_equal(got["n_below"][s], want[tile]["n_below"][s]), (tile, s)
    assert np.array_equal(d_score.view(torch.int32).cpu().numpy(), before) and np.array_equal(before.view(np.uint32), score.view(np.uint32))


@pytest.mark.parametrize("name", ["random_bits", "ties"])
@pytest.mark.parametrize("film", [(7, 3), (9, 9), (65, 33), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_unaligned_images_take_the_element_path_to_the_same_bits(gpu, film, name):
    score, want = case(film, name)
    d_score = dev_offset(score)
    for tile in ref.TILES:
        assert_planes(run(gpu, d_score, tile), want[tile], (film, name, tile))


def shuffled_within_tiles(score, tile, seed=3):
    rng = np.random.default_rng(seed)
    out = np.array(score)
    H, W = out.shape
    for y in range(0, H, tile):
        for x in range(0, W, tile):
            block = out[y:y + tile, x:x + tile]
            out[y:y + tile, x:x + tile] = rng.permutation(block.reshape(-1)).reshape(block.shape)
    return out


@pytest.mark.parametrize("name", ["random_bits", "ties"])
@pytest.mark.parametrize("film", [(67, 130), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_two_runs_and_a_shuffle_within_tiles_give_the_same_bits(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    for tile in ref.TILES:
        first = run(gpu, d_score, tile)
        assert_planes(run(gpu, d_score, tile), first, (film, name, tile, "again"))
        moved = shuffled_within_tiles(score, tile)
        assert not np.array_equal(moved.view(np.uint32), score.view(np.uint32))
        assert_planes(run(gpu, dev(moved), tile), want[tile], (film, name, tile, "shuffled"))


# ---------------------------------------------------------------- 3. the other entries on the same data
@pytest.mark.parametrize("name", ["random_bits", "ties", "all_infinite"])
def test_the_maximum_is_score_tiles_and_the_planes_are_score_images(gpu, name):
    import torch
    score, want = case((257, 70), name)
    d_score = dev(score)
    for tile in ref.TILES:
        res = gpu.score_tile_select(d_score, tile, NUMS, DEN, fields=("value",))
        top = gpu.score_tiles(d_score, tile, planes=("max",))["max"]
        torch.cuda.synchronize()
        assert np.array_equal(res["value"][3].cpu().numpy().view(np.uint32), top.cpu().numpy().view(np.uint32)), tile
        plane = want[tile]["value"][2]
        keys = np.sort(plane.view(np.uint32).reshape(-1))
        thresholds = [from_bits([int(keys[keys.size // 2])])[0], F32(0.0), F32(0.02), from_bits([int(keys[-1])])[0]]
        above = gpu.score_count_above(res["value"][2], thresholds).cpu().numpy()
        assert [int(v) for v in above] == [int((keys > sel_ref.key_of(t)).sum()) for t in thresholds], tile
        ranks = [0, keys.size // 2, keys.size - 1]
        assert gpu.read_select_result(gpu.score_select(res["value"][2], ranks))["value_bits"] == [int(keys[r]) for r in ranks], tile


@pytest.mark.parametrize("name", ["random_bits", "ties", "all_infinite"])
@pytest.mark.parametrize("film", [f for f in FILMS if f[0] <= 64 and f[1] <= 64], ids=lambda f: "%dx%d" % f)
def test_one_tile_over_the_film_is_score_select(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    W, H = film
    ranks = [ref.rank_of(W * H, num, DEN) for num in NUMS]
    sel = gpu.read_select_result(gpu.score_select(d_score, ranks))
    got = run(gpu, d_score, 64)
    for s in range(4):
        assert got["value"][s].shape == (1, 1)
        assert (int(got["value"][s].view(np.uint32)[0, 0]), int(got["n_below"][s][0, 0]), int(got["n_equal"][s][0, 0])) == \
               (sel["value_bits"][s], sel["n_below"][s], sel["n_equal"][s]), (film, name, s)


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(16, 16, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="tile = 12"):
        gpu.score_tile_select(score, 12, [1], 2)
    with pytest.raises(gpu.StatmcError, match="q_den = 0"):
        gpu.score_tile_select(score, 8, [0], 0)
    with pytest.raises(gpu.StatmcError, match=r"q_num\[1\] = 3"):
        gpu.score_tile_select(score, 8, [0, 3], 2)
    with pytest.raises(gpu.StatmcError, match="every plane"):
        gpu.score_tile_select(score, 8, [1], 2, fields=())
    with pytest.raises(gpu.StatmcError, match=r"out->value\[0\] overlaps score"):
        gpu.score_tile_select(score, 8, [1], 2, fields=("value",), out={"value": [score.view(-1)[:4].view(2, 2)]})
    value = torch.ones(2, 2, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="threshold is NaN"):
        gpu.gate_tiles(16, 16, 8, value, float("nan"))
    with pytest.raises(gpu.StatmcError, match="tile = 4"):
        gpu.gate_tiles(16, 16, 4, torch.ones(4, 4, device="cuda:0"), 1.0)
    with pytest.raises(gpu.StatmcError, match="closed overlaps tile_value"):
        gpu.gate_tiles(16, 16, 8, value, 1.0, closed=value.view(torch.int32))
    both = torch.zeros(16 * 16 + 4, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match=r"dst\[0\] overlaps src\[0\]"):
        gpu.gate_tiles(16, 16, 8, value, 1.0, images=[both[:256].view(16, 16)], out=[both[4:].view(16, 16)])


# ---------------------------------------------------------------- 4. the gate
GATE_FILMS = [(1, 1), (7, 3), (9, 9), (65, 33), (67, 130), (257, 70)]


def gate_inputs(film, tile, seed=0):
    """(tile values, threshold, a float image, an int32 image, two more images) of a film"""
    W, H = film
    rng = np.random.default_rng(W * 100 + H + tile + seed)
    ty, tx = -(-H // tile), -(-W // tile)
    values = rng.choice(np.array([0, 0x3C23D70A, 0x3CA3D70A, 0x3CA3D70B, 0x3F800000, 0x7F800000, 0xFFC00000, 0x80000001], np.uint32), (ty, tx))
    scores = from_bits(rng.integers(1, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32))
    counts = rng.integers(-3, 50, (H, W)).astype(np.int32)
    more = [from_bits(rng.integers(1, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)), rng.integers(1, 9, (H, W)).astype(np.int32)]
    return from_bits(values), float(from_bits([0x3CA3D70A])[0]), scores, counts, more


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("film", GATE_FILMS, ids=lambda f: "%dx%d" % f)
def test_the_gate_equals_the_restatement_in_and_out_of_place(gpu, film):
    import torch
    W, H = film
    for tile in ref.TILES:
        values, thr, scores, counts, more = gate_inputs(film, tile)
        ty, tx = values.shape
        closed0 = (np.random.default_rng(tile).integers(0, 3, (ty, tx)) == 0).astype(np.int32) * 9
        for closed in (None, closed0):
            for images in ([], [scores], [scores, counts] + more):
                o, c, res, gated = ref.gate_ref(H, W, tile, values, thr, closed, images)
                for place in ("out", "in"):
                    d_images = [dev(im) for im in images]
                    d_closed = None if closed is None else dev(closed)
                    d_open = torch.full((ty, tx), 5, dtype=torch.int32, device="cuda:0")
                    got_open, got_images, result = gpu.gate_tiles(H, W, tile, dev(values), thr, closed=d_closed, open=d_open, images=d_images,
                                                                  out=d_images if place == "in" else None)
                    what = (film, tile, closed is not None, len(images), place)
                    assert gpu.read_gate_result(result) == res, what
                    assert np.array_equal(got_open.cpu().numpy(), o), what
                    if closed is not None:
                        assert np.array_equal(d_closed.cpu().numpy(), c), what
                    for k, im in enumerate(images):
                        assert got_images[k].dtype == d_images[k].dtype
                        assert np.array_equal(words(got_images[k].cpu().numpy()), gated[k]), what + (k,)
                        if place == "out":
                            assert np.array_equal(words(d_images[k].cpu().numpy()), words(im)), what + (k, "the source is only read")
        # an image 4 bytes off 16-byte alignment takes the element path
        o, c, res, gated = ref.gate_ref(H, W, tile, values, thr, None, [scores, counts])
        _, got_images, _ = gpu.gate_tiles(H, W, tile, dev(values), thr, images=[dev_offset(scores), dev(counts)])
        assert all(np.array_equal(words(g.cpu().numpy()), w) for g, w in zip(got_images, gated)), (film, tile, "offset")


def test_a_closed_tile_stays_closed_over_three_calls(gpu):
    import torch
    W, H, tile = 257, 70, 16
    ty, tx = gpu.tile_grid(H, W, tile)
    rng = np.random.default_rng(5)
    first = rng.uniform(0.0, 0.04, (ty, tx)).astype(F32)
    planes = [first, (first * F32(0.75)).astype(F32), (first * F32(4.0)).astype(F32)]      # falling, then rising above the start
    thr = 0.02
    closed = np.zeros((ty, tx), np.int32)
    d_closed = torch.zeros(ty, tx, dtype=torch.int32, device="cuda:0")
    history = []
    for k, plane in enumerate(planes):
        o, closed, res, _ = ref.gate_ref(H, W, tile, plane, thr, closed, [])
        got_open, _, result = gpu.gate_tiles(H, W, tile, dev(plane), thr, closed=d_closed)
        got = gpu.read_gate_result(result)
        assert got == res and np.array_equal(got_open.cpu().numpy(), o) and np.array_equal(d_closed.cpu().numpy(), closed), k
        history.append(got)
    assert history[0]["n_closed_now"] > 0 and history[1]["n_closed_now"] > 0 and history[2]["n_closed_now"] == 0
    assert history[0]["n_open"] > history[1]["n_open"] == history[2]["n_open"] > 0      # the rising plane reopens nothing
    assert sum(h["n_closed_now"] for h in history) == ty * tx - history[2]["n_open"]
    assert int(((planes[2] > F32(thr)) & (closed != 0)).sum()) > 0      # tiles above the threshold again, and closed all the same


def test_the_open_plane_and_the_gated_images_go_through_compact_offsets_and_plan_samples(gpu):
    import torch
    W, H, tile = 257, 70, 16
    values, thr, _, _, _ = gate_inputs((W, H), tile, seed=1)
    ty, tx = values.shape
    rng = np.random.default_rng(9)
    scores = rng.uniform(0.001, 1.0, (H, W)).astype(F32)
    o, _, res, gated = ref.gate_ref(H, W, tile, values, thr, None, [scores])
    d_open, (d_gated,), result = gpu.gate_tiles(H, W, tile, dev(values), thr, images=[dev(scores)])
    offsets, owners = gpu.compact_offsets(d_open, cap=1, owners_capacity=ty * tx)      # the open tiles, in raster order
    torch.cuda.synchronize()
    open_tiles = np.flatnonzero(o.reshape(-1))
    assert int(offsets[-1].item()) == open_tiles.size == res["n_open"] and 0 < open_tiles.size < ty * tx
    assert np.array_equal(owners.cpu().numpy()[:open_tiles.size], open_tiles) and np.all(owners.cpu().numpy()[open_tiles.size:] == -1)
    # a plan on the gated score with c_min = 0: the budget goes to the open tiles alone, to the sample
    keep = o.reshape(-1)[ref.tile_of_pixels(H, W, tile)].astype(bool)
    budget = 4 * res["n_px_open"]
    counts, plan = gpu.plan_samples(d_gated, budget, 0, 64, return_result=True)
    host = counts.cpu().numpy()
    assert int(host.sum()) == plan["total"] == budget and np.all(host[~keep] == 0) and int(keep.sum()) == res["n_px_open"]
    # a count image planned with c_min = 2 and gated afterwards: exactly 0 in closed tiles, the restated total
    counts2 = gpu.plan_samples(dev(scores), 6 * W * H, 2, 64)
    host2 = counts2.cpu().numpy()
    assert host2.min() >= 2
    _, (d_counts2,), _ = gpu.gate_tiles(H, W, tile, dev(values), thr, images=[counts2], out=[counts2])
    offsets2, _ = gpu.compact_offsets(d_counts2)
    torch.cuda.synchronize()
    assert np.array_equal(d_counts2.cpu().numpy(), np.where(keep, host2, 0)) and int(offsets2[-1].item()) == int(host2[keep].sum())


def test_a_quantile_plane_gates_a_film(gpu):
    """the pieces together: the 95th percentile per tile, the gate at 2 %, on an error-like image with a converged half"""
    score, _ = case((257, 70), "random_bits")
    rng = np.random.default_rng(12)
    err = rng.uniform(0.0, 0.03, (70, 257)).astype(F32)
    err[:, :120] *= F32(0.3)
    err[5, 7] = INF
    for tile in ref.TILES:
        w = ref.tile_select_ref(err, tile, [19], 20)
        res = gpu.score_tile_select(dev(err), tile, [19], 20, fields=("value",))
        o, _, want, gated = ref.gate_ref(70, 257, tile, w["value"][0], 0.02, None, [err])
        d_open, (d_err,), result = gpu.gate_tiles(70, 257, tile, res["value"][0], 0.02, images=[dev(err)])
        assert gpu.read_gate_result(result) == want and 0 < want["n_open"] < want["n_tiles"], tile
        assert np.array_equal(d_open.cpu().numpy(), o) and np.array_equal(words(d_err.cpu().numpy()), gated[0]), tile


# ---------------------------------------------------------------- 5. the stream contract
def test_both_entries_run_on_their_stream_and_an_event_makes_the_results_visible(gpu):
    """The gate of tests/test_stream_contract_gpu.py: on a non-blocking library stream, the inputs and outputs full of poison are
    overwritten behind a closed gate, then the entry, then the read-back, all on that stream -- anything the entry put on another
    stream would see the poison.  Then an event recorded behind a second call on the side stream, which the null stream waits for."""
    import torch
    from test_stream_contract_gpu import Case, assert_same_bits, run_gated, run_on_null_stream, stream_apart_from_the_null_stream
    api, lib = gpu, gpu.load()
    film, tile = (257, 70), 16
    W, H = film
    score, want = case(film, "random_bits")
    other, _ = case(film, "ties")
    w = want[tile]
    ty, tx = w["value"][0].shape
    values, thr, scores, counts, _ = gate_inputs(film, tile)
    closed0 = (np.random.default_rng(3).integers(0, 3, (ty, tx)) == 0).astype(np.int32)
    o, c_after, res, gated = ref.gate_ref(H, W, tile, values, thr, closed0, [scores, counts])
    assert torch.cuda.current_stream().cuda_stream == 0
    side, gate = stream_apart_from_the_null_stream(api)
    event = C.c_void_p()
    api.check(lib.statmc_event_create(C.byref(event)))
    try:
        c = Case("score_tile_select-257x70")
        d_score = c.live(np.array(score), b=np.array(other))
        out = {f: [c.live(np.zeros((ty, tx), w[f][s].dtype), b=np.full((ty, tx), 5, w[f][s].dtype), out="%s%d" % (f, s)) for s in range(4)] for f in ref.FIELDS}
        c.call = lambda stream: api.score_tile_select(d_score, tile, NUMS, DEN, out=out, stream=stream)
        on_null = run_on_null_stream(c)
        gated_run = run_gated(api, c, side, gate)
        assert_same_bits(c, gated_run, on_null, "gated on the side stream against the null-stream run")
        assert_planes({f: [c.res("%s%d" % (f, s)) for s in range(4)] for f in ref.FIELDS}, w, "gated")

        g = Case("gate_tiles-257x70")
        d_values = g.live(np.array(values), b=np.full(values.shape, INF, F32))
        d_closed = g.live(closed0, b=np.full((ty, tx), 1, np.int32), out="closed")
        d_open = g.live(np.zeros((ty, tx), np.int32), b=np.full((ty, tx), 5, np.int32), out="open")
        d_scores = g.live(np.array(scores), b=np.full((H, W), 3.0, F32))
        d_counts = g.live(np.array(counts), b=np.full((H, W), 77, np.int32), out="counts")      # in place
        d_gated = g.live(np.zeros((H, W), F32), b=np.full((H, W), 3.0, F32), out="gated")
        d_result = g.live(np.zeros(4, np.int64), b=np.full(4, 5, np.int64), out="result")
        g.call = lambda stream: api.gate_tiles(H, W, tile, d_values, thr, closed=d_closed, open=d_open, images=[d_scores, d_counts],
                                               out=[d_gated, d_counts], result=d_result, stream=stream)
        on_null = run_on_null_stream(g)
        gated_run = run_gated(api, g, side, gate)
        assert_same_bits(g, gated_run, on_null, "gated on the side stream against the null-stream run")
        assert np.array_equal(g.res("open"), o) and np.array_equal(g.res("closed"), c_after)
        assert np.array_equal(words(g.res("gated")), gated[0]) and np.array_equal(words(g.res("counts")), gated[1])
        assert g.res("result").tolist() == [res["n_tiles"], res["n_open"], res["n_closed_now"], res["n_px_open"]]
        # the event
        for ts in out.values():
            for t in ts:
                t.fill_(5)
        torch.cuda.synchronize()
        c.call(side.handle)
        api.check(lib.statmc_event_record(event, side.handle))
        api.check(lib.statmc_stream_wait_event(None, event))
        seen = {f: [t.clone() for t in ts] for f, ts in out.items()}      # on the null stream, behind the event
        torch.cuda.current_stream().synchronize()
        assert_planes({f: [t.cpu().numpy() for t in ts] for f, ts in seen.items()}, w, "behind the event")
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_event_destroy(event))
        side.destroy()


# ---------------------------------------------------------------- 6. FilmStats
def test_film_stats_tile_quantiles_and_gate_on_an_accumulated_film(gpu):
    import torch
    from statmc_amd.film import FilmStats
    W, H = 64, 48
    names = ("radiance", "normal", "albedo")
    _, smp, _ = make_case(W, H, 9)
    rng = np.random.default_rng(17)
    counts = rng.integers(2, 10, (H, W)).astype(np.int32)
    counts.reshape(-1)[::11] = rng.integers(0, 2, counts.reshape(-1)[::11].size)
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names}, counts=dev(counts))
    rad = film.state["radiance"]
    score = gpu.error_scores(rad["n"], rad["film_mean"], rad["film_m2"], metric="relative", eps=1e-3, table="stderr").cpu().numpy()
    assert int(np.isinf(score).sum()) == int((counts < 2).sum()) > 100
    for tile in ref.TILES:
        got = film.score_tile_quantiles(tile, [0.5, (19, 20), 1.0, (0, 1)])
        torch.cuda.synchronize()
        assert_planes(gpu.read_tile_quantiles(got), ref.tile_select_ref(score, tile, [10, 19, 20, 0], 20), tile)
    got = film.score_tile_quantiles(16, [(1, 3), 0.75], fields=("value",))      # brought to twelfths
    assert_planes(gpu.read_tile_quantiles(got), ref.tile_select_ref(score, 16, [4, 9], 12), "twelfths", slots=range(2), fields=("value",))
    with pytest.raises(ValueError, match="common denominator"):
        film.score_tile_quantiles(16, [(1, 65521), (1, 65519)])
    median = got["value"][0]
    thr = float(np.median(median.cpu().numpy()))
    closed = torch.zeros(3, 4, dtype=torch.int32, device="cuda:0")
    is_open, (gated,), res = film.gate_tiles(16, median, thr, closed=closed, images=[dev(score)])
    o, c, want, g = ref.gate_ref(H, W, 16, median.cpu().numpy(), thr, np.zeros((3, 4), np.int32), [score])
    assert res == want and 0 < res["n_open"] < 12 and np.array_equal(is_open.cpu().numpy(), o) and np.array_equal(closed.cpu().numpy(), c)
    assert np.array_equal(words(gated.cpu().numpy()), g[0])


# ---------------------------------------------------------------- 7. the render loop
def run_sim(build, stem, *extra):
    import subprocess
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "96", "--height", "64", "--spp", "4", "--iterations", "4", "--threads", "4",
                          "--adaptive-pixels", "--stop-metric", "stderr", "--stem", stem] + list(extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_render_loop_closes_tiles_by_their_quantile(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels --stop-tiles 16:TOL --tile-quantile 19/20 --close-tiles on 96 x 64, four iterations.  TOL is
    the median of the first iteration's restated quantile plane (from the statistics a run that never stops dumped), so about half
    the tiles close at once.  The "Closed tiles:" lines are consistent, the first equals the restated gate, and every later
    iteration spends at most the schedule's samples per pixel times the open pixels before it."""
    import re
    import subprocess
    from statmc_amd import build, pfm
    import error_reference as err_ref
    import plan_reference as plan_ref
    build.build_tools()
    W, H, tile = 96, 64, 16
    rule = re.compile(r"^Tile rule: iteration (\d+), open tiles (\d+) / (\d+) of 16 x 16 pixels, quantile 19/20 of the relative standard error above (\S+): (met|open)$", re.M)
    closed_line = re.compile(r"^Closed tiles: iteration (\d+), closed now (\d+), open (\d+) / (\d+), open pixels (\d+)$", re.M)

    never = run_sim(build, str(tmp_path / "never"), "--stop-tiles", "16:0", "--tile-quantile", "19/20")
    assert len(rule.findall(never)) == 4 and "Closed tiles:" not in never
    rd = lambda what: np.asarray(pfm.read_pfm("%s-4-t0-b0-%s.pfm" % (str(tmp_path / "never"), what)))
    score = err_ref.error_scores_ref(rd("n").astype(np.int32), rd("film-mean"), rd("film-m2"), plan_ref.RELATIVE, 1e-3, None)
    plane = ref.tile_select_ref(score, tile, [19], 20)["value"][0]
    assert int(rule.findall(never)[0][1]) == int((sel_ref.keys_of(plane) > 0).sum())
    tol = float(np.median(plane))
    o, _, want, _ = ref.gate_ref(H, W, tile, plane, tol, np.zeros(plane.shape, np.int32), [])
    assert 0 < want["n_open"] < want["n_tiles"] == 24

    out = run_sim(build, str(tmp_path / "close"), "--stop-tiles", "16:%.9g" % tol, "--tile-quantile", "19/20", "--close-tiles")
    lines = [tuple(int(v) for v in m) for m in closed_line.findall(out)]
    n_iter = len(re.findall(r"^Iteration: ", out, re.M))
    assert len(lines) == n_iter >= 2 and [l[0] for l in lines] == list(range(1, n_iter + 1)), out
    assert lines[0][1:] == (want["n_closed_now"], want["n_open"], 24, want["n_px_open"]), (lines[0], want)
    opens = [l[2] for l in lines]
    assert all(a >= b for a, b in zip(opens, opens[1:])) and sum(l[1] for l in lines) == 24 - opens[-1]      # open never rises
    assert all(l[4] <= l[2] * tile * tile for l in lines) and (opens[-1] == 0 or n_iter == 4)
    spent = [int(v) for v in re.findall(r"^Spent: (\d+) samples$", out, re.M)]
    assert len(spent) == n_iter and spent[0] == 4 * W * H
    for k in range(1, n_iter):
        sched = 4 << max(k - 1, 0)      # the schedule's samples per pixel of iteration k + 1
        assert 0 < spent[k] <= sched * lines[k - 1][4], (k, spent[k], sched, lines[k - 1])
    # without the new flags: the mean rule's lines, no gate
    plain = run_sim(build, str(tmp_path / "plain"), "--stop-tiles", "16:0")
    assert "Closed tiles:" not in plain and "quantile 19/20" not in plain and len(re.findall(r"^Tile rule: .* mean of the relative standard error under inf above 0: open$", plain, re.M)) == 4
    assert re.findall(r"^Spent: (\d+) samples$", plain, re.M) == [str(s * W * H) for s in (4, 4, 8, 16)]
    for bad in (["--adaptive-pixels", "--tile-quantile", "19/20"], ["--adaptive-pixels", "--close-tiles"],
                ["--adaptive-pixels", "--stop-tiles", "16:1", "--tile-quantile", "21/20"], ["--adaptive-pixels", "--stop-tiles", "16:1", "--tile-quantile", "0.95"],
                ["--adaptive-pixels", "--stop-tiles", "16:1", "--close-tiles", "--target-error", "0.1"]):
        r = subprocess.run([build.RENDER_SIM_BIN, "--width", "16", "--height", "16"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and ("--tile-quantile" in r.stderr or "--close-tiles" in r.stderr), (bad, r.stderr)
