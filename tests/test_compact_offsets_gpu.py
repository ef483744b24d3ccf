"""statmc_compact_offsets on the GPU: offsets and owners equal the numpy restatement (tests/compact_reference.py) -- integer sums,
so equal means the same bits -- for ragged, negative, capped, empty and misaligned count images, at every relation of
owners_capacity to the total, on every run, and for the count image statmc_plan_samples writes."""
import numpy as np
import pytest

import compact_reference as ref
import plan_reference
from test_records_gpu import FILMS, dev, ragged_counts

pytestmark = pytest.mark.gpu

SENTINEL = -77


def run_offsets(api, counts, cap=None, owners_capacity=0, misalign=False):
    """-> (offsets, owners, the element just past owners_capacity) as numpy; the owners tensor is one entry longer than the
    capacity and holds a sentinel there.  misalign: the count image starts 4 bytes into its allocation."""
    import torch
    H, W = counts.shape
    if misalign:
        raw = torch.zeros(H * W + 1, dtype=torch.int32, device="cuda:0")
        d_counts = raw[1:].view(H, W)
        d_counts.copy_(dev(counts))
        assert d_counts.data_ptr() % 16 == 4
    else:
        d_counts = dev(counts)
    owners = torch.full((owners_capacity + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    offsets = torch.full((H * W + 1,), -1, dtype=torch.int64, device="cuda:0")
    got_offsets, got_owners = api.compact_offsets(d_counts, cap=cap, owners_capacity=owners_capacity, out=(offsets, owners if owners_capacity else None))
    torch.cuda.synchronize()
    assert got_offsets is offsets
    own = owners.cpu().numpy()
    return offsets.cpu().numpy(), own[:owners_capacity], int(own[owners_capacity])


def check(api, counts, cap=None, capacities=None, misalign=False):
    want = ref.offsets_ref(counts, ref.INT32_MAX if cap is None else cap)
    total = int(want[-1])
    for capacity in (capacities if capacities is not None else (total + 9,)):
        offsets, owners, past = run_offsets(api, counts, cap, capacity, misalign)
        assert offsets.dtype == np.int64 and np.array_equal(offsets, want), (capacity, int((offsets != want).sum()))
        assert np.array_equal(owners, ref.owners_ref(counts, capacity, ref.INT32_MAX if cap is None else cap)), capacity
        assert past == SENTINEL, capacity
    return total


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_ragged_counts_at_every_owners_capacity(gpu, film):
    W, H = film
    counts = ragged_counts(np.random.default_rng(40 + W), W * H).astype(np.int32).reshape(H, W)
    assert counts.max() == 300 and (counts == 0).mean() > 0.1
    total = int(counts.sum())
    # below, equal to and above the total; 0: no owners at all
    assert check(gpu, counts, capacities=(0, 1, total - 301, total - 1, total, total + 1, total + 1000)) == total


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_negative_counts_and_counts_above_the_cap(gpu, film):
    W, H = film
    rng = np.random.default_rng(50 + W)
    counts = rng.integers(-20, 40, (H, W)).astype(np.int32)
    counts.reshape(-1)[::97] = np.iinfo(np.int32).min
    counts.reshape(-1)[5::101] = np.iinfo(np.int32).max
    for cap in (12, 1, 0):
        total = check(gpu, counts, cap=cap)
        assert total == int(np.clip(counts.astype(np.int64), 0, cap).sum())
    assert check(gpu, counts, cap=0) == 0
    # no cap: the int32 maxima add up beyond 2^31 in the int64 sums; the owners are cut at their capacity
    want = ref.offsets_ref(counts)
    assert int(want[-1]) > 2 ** 33
    offsets, owners, past = run_offsets(gpu, counts, None, 5000)
    assert np.array_equal(offsets, want) and np.array_equal(owners, ref.owners_ref(counts, 5000)) and past == SENTINEL


def test_every_count_zero(gpu):
    W, H = FILMS[0]
    offsets, owners, past = run_offsets(gpu, np.zeros((H, W), np.int32), None, 50)
    assert not offsets.any() and np.all(owners == -1) and past == SENTINEL


def test_a_three_pixel_film(gpu):
    assert check(gpu, np.array([[2, 0, 5]], np.int32), capacities=(0, 3, 7, 12)) == 7
    assert check(gpu, np.array([[0, 0, 1]], np.int32), capacities=(1, 2)) == 1


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_a_count_image_four_bytes_into_its_allocation(gpu, film):
    W, H = film
    counts = ragged_counts(np.random.default_rng(60 + W), W * H).astype(np.int32).reshape(H, W)
    check(gpu, counts, misalign=True)


def test_several_scan_blocks_and_a_second_step_of_the_block_scan(gpu):
    """1024 pixels per scan block, 256 block sums per step of the one-workgroup scan: 600 x 500 pixels are 293 blocks."""
    W, H = 600, 500
    counts = np.random.default_rng(8).integers(-3, 6, (H, W)).astype(np.int32)
    counts[H - 1, W - 1] = 1000
    total = check(gpu, counts, capacities=(4097,))
    assert total == int(np.clip(counts, 0, None).sum())


def test_two_runs_give_the_same_bits(gpu):
    W, H = FILMS[1]
    counts = ragged_counts(np.random.default_rng(3), W * H).astype(np.int32).reshape(H, W)
    a = run_offsets(gpu, counts, 7, 3000)
    b = run_offsets(gpu, counts, 7, 3000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_the_offsets_of_a_plan_end_in_exactly_the_budget(gpu, film):
    W, H = film
    score = plan_reference.lognormal_scores(H, W, 1)
    budget = W * H * 6 + 11
    counts, result = gpu.plan_samples(dev(score), budget, 1, 64, return_result=True)
    assert result["status"] == 0 and result["total"] == budget
    offsets, owners = gpu.compact_offsets(counts, owners_capacity=budget)
    o, own = offsets.cpu().numpy(), owners.cpu().numpy()
    assert int(o[-1]) == budget and o[0] == 0
    assert np.array_equal(o, ref.offsets_ref(counts.cpu().numpy()))
    assert own.min() >= 0 and np.array_equal(np.bincount(own, minlength=W * H), counts.cpu().numpy().reshape(-1))
