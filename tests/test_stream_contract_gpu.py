"""The stream contract of include/statmc.h -- "every call is asynchronous on `stream`" -- held for every entry point that
takes a stream, on a NON-BLOCKING side stream, where nothing orders itself by accident against the null stream.

The gate.  Every table row runs this sequence, all of it enqueued on the side stream `s` (statmc_stream_create) while
torch's current stream stays the null stream:

    1. a spin of GATE_PROBES statmc_clock_probe launches of PROBE_CYCLES shader clocks each; event e_gate behind it
    2. copies of input set A and of the start state from staging tensors into the live tensors (which hold input set B and
       junk, both valid data, put there on the null stream before a device-wide synchronisation)
    3. the entry under test, stream = s
    4. copies of every output / state image into result tensors

Right after the last enqueue the host asserts that e_gate has NOT fired: the gate was still closed, so nothing of 2 - 4 can
have run.  Anything the entry puts on another stream (a launch, memset or copy on the null stream, a wrapper that drops its
stream=, a helper stream without an event edge back to s) runs while the gate is closed: it reads B or junk, or what it
writes is overwritten by the late copy of A.  Either way the result is not f(A), and the row compares every plane with
f(A) as int32 bit patterns, NaN payloads included.  f(A) is the same entry run on the null stream with A resident -- the
path the rest of the suite ties to the CPU oracle -- and, where the suite has an oracle helper for the entry, the gated
result is held to the oracle on A as well (the accumulation family through test_records_gpu.assert_matches_the_oracle,
pre-pass, prepass-pack, merge-tiles, mean-vars, tile-moments, film-update bit for bit, the window filter through
test_gpu_parity.assert_per_pixel).  A gate that had opened early FAILS the row with a message saying so.

Two controls show that the harness sees a wholly misplaced call: statmc_prepass and statmc_accumulate enqueued on the null
stream while their inputs are gated on s return f(B) != f(A), and the untouched start state, bit for bit.

Safety of the poison: B and the junk are valid data (record pixels inside the film, finite floats, small counts); every
table a kernel dereferences through (tile bounds / offsets / samples per tile, record layouts) is resident and never gated.

Gate length.  statmc_clock_probe accepts at most 2^24 shader clocks per launch (about 7 ms), so the gate is a chain of
launches on s: G = GATE_PROBES x PROBE_CYCLES = 16 x 2^24 = 2^28 shader clocks, below the 2^30 the harness allows itself.
Measured on an MI355X (test_enqueue_times_and_gate_length prints the table): host time to enqueue copy-in, entry and
read-back of a row on the null stream, second pass (the first sizes workspaces and caches tables, as the gated run's warm-up
does; first passes took up to 8.5 ms, statmc_accumulate_records allocating its workspace), and from closing the gate to
the last enqueue behind it, the 16 gate launches included:

    row                                     null stream   behind the gate
    combine_many-7x3-K5 (285 gated images)      1367 us           1480 us
    records_split-37x29                          299 us            458 us
    accumulate_tiles-37x29                       262 us            417 us
    records-37x29                                262 us            348 us
    accumulate_plain-37x29                       211 us            691 us
    the other accumulation and records rows  174 - 240 us      307 - 394 us
    combine_statistics-7x3                       187 us            317 us
    window_filter-float5                         120 us            257 us
    prepass_pack                                  96 us            638 us
    filter_f32 / filter_f32x3                     69 us       205 - 209 us
    window_filter-pitched                         59 us            191 us
    the other filter and pack rows            30 - 62 us      131 - 207 us
    pointwise rows, copies                    19 - 59 us      148 - 189 us

    the 16 probes' elapsed constant-rate clock (the sum of their out[1]): 109.9 - 112.0 ms per gate, 2.4 GHz shader clock
    = 76 - 80 x the slowest row on the null stream (two runs), 74 x the slowest gated enqueue, 13 x the slowest first pass

The gate must last at least 20 x the slowest row; G = 2^28 leaves four times that.

The two-streams-released-together part (test_two_streams_released_together) is PROBABILISTIC: both streams start in the
same instant behind one gate, but whether their kernels really overlap is the hardware's choice.  It exists to catch scratch
keyed by device only; a pass does not prove the absence of sharing, a failure proves sharing.

At most three library streams are alive at any time: the HIP runtime opens four hardware queues per process by default
(GPU_MAX_HW_QUEUES), and a gated stream must not share a queue with the stream it is meant to race against.  The streams
that race against the null stream -- the table's and the controls' stream, the cold row's -- are therefore taken from
stream_apart_from_the_null_stream(), which shows that they do not share its queue.  (In a run of the whole suite, which has
made dozens of streams before this file starts, the cold row's first candidate did share it: the synchronous table upload
of the cold call, on the null stream, then waited for the gate, and the host with it -- 111.8 ms to enqueue, the length of
the gate.  The results were right; the row rightly refused to count them.)

What the gate cannot see: an operation that neither reads gated data nor has its writes overwritten by the late copy -- a
scratch memset that runs early instead of in stream order leaves the same zeros.  What it was shown to see, each by a
deliberately wrong build while this file was written: the records' segments kernel launched on the null stream, the
copy of a pitched image into its packed twin issued on the null stream, and api.combine_many / api.tile_moments dropping
their stream= -- the rows of exactly those entries failed with "differs in ... elements", every other row passed."""
import contextlib
import ctypes as C
import functools
import time
import types as pytypes

import numpy as np
import pytest
import torch

from conftest import FILTER_SD, RADIUS, SD_ALBEDO, SD_NORMAL, make_case
from test_gpu_parity import assert_per_pixel
from test_records_gpu import TYPES, assert_matches_the_oracle, make_samples, ragged_counts, records_of_counts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G_DR = [-0.5 / SD_NORMAL ** 2, -0.5 / SD_ALBEDO ** 2]
PROBE_CYCLES = 1 << 24       # the most one statmc_clock_probe launch spins
GATE_PROBES = 16             # launches per gate: 2^28 shader clocks in all
SENTINEL = -7.0
ENQUEUE_US = {}              # row -> host microseconds to enqueue copy-in, entry and read-back on the null stream
GATED_US = {}                # row -> host microseconds from closing the gate to the last enqueue behind it
GATE_TICKS = []              # 10 ns ticks of every gate that was closed
SET_ASIDE = []               # the streams that shared the null stream's hardware queue (their priority class)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype == np.float32:
        return a.view(np.int32)
    if a.dtype == np.float16:
        return a.view(np.int16)
    return a


def junk_like(rng, a):
    """Valid data of a's shape and type that is not a: finite floats, small non-negative counts, any bytes."""
    if a.dtype == np.int32:
        return rng.integers(0, 1000, a.shape).astype(np.int32)
    if a.dtype == np.uint8:
        return rng.integers(0, 256, a.shape).astype(np.uint8)
    return rng.normal(0.0, 1.0, a.shape).astype(a.dtype)


class SideStream:
    """A library stream (statmc_stream_create: non-blocking) and torch's view of it.  priority_class: a stream of another
    priority class (statmc_stream_create_with_priority), which never shares a hardware queue with normal streams."""

    def __init__(self, api, priority_class=None):
        self.api, self.lib = api, api.load()
        self.handle = C.c_void_p()
        if priority_class is None:
            api.check(self.lib.statmc_stream_create(C.byref(self.handle)))
        else:
            api.check(self.lib.statmc_stream_create_with_priority(C.byref(self.handle), priority_class))
        self.ext = torch.cuda.ExternalStream(self.handle.value)

    def synchronize(self):
        self.api.check(self.lib.statmc_synchronize(self.handle))

    def destroy(self):
        if self.handle:
            self.api.check(self.lib.statmc_stream_destroy(self.handle))
            self.handle = C.c_void_p()


class Gate:
    """GATE_PROBES one-wave spins in a row on a stream; closed() tells whether the last of them is still running."""

    def __init__(self):
        self.out = torch.zeros(GATE_PROBES, 2, dtype=torch.int64, device=DEV)
        self.event = torch.cuda.Event()

    def close(self, api, side):
        for i in range(GATE_PROBES):
            api.clock_probe(self.out[i], cycles=PROBE_CYCLES, stream=side.handle)
        self.event.record(side.ext)

    def closed(self):
        return not self.event.query()

    def ticks(self):
        return int(self.out[:, 1].sum().item())


def stream_apart_from_the_null_stream(api, candidates=(None, None, 1)):
    """A side stream and its gate, shown NOT to share a hardware queue with the null stream: with the gate closed on it, a
    kernel on the null stream runs to its end.  The runtime deals its streams over a few hardware queues, and every packet
    waits for the one before it in its queue: behind a closed gate in the null stream's queue, null-stream work -- a
    control's misplaced call, the synchronous table upload of a cold filter call -- would wait for the gate, and the test
    that counts on it running early would report an open gate.  Which queue a new stream gets depends on the streams the
    process has made before, so a stream that shares is set aside (kept alive, so that the next one gets another queue)
    and the last candidate comes from another priority class, whose queues are not the null stream's."""
    set_aside = []
    scratch = torch.zeros(64, device=DEV)
    torch.cuda.synchronize()
    try:
        for priority_class in candidates:
            side, gate = SideStream(api, priority_class), Gate()
            gate.close(api, side)
            scratch.add_(1.0)                                  # on the null stream
            torch.cuda.current_stream().synchronize()
            apart = gate.closed()
            side.synchronize()
            if apart:
                return side, gate
            set_aside.append(side)
            SET_ASIDE.append(priority_class)
        raise AssertionError("no stream apart from the null stream's hardware queue: every candidate shared it")
    finally:
        for side in set_aside:
            side.destroy()


class Case:
    """One table row: live tensors (what the entry reads and writes), their staged A / start values, their poison (B / junk),
    the entry call and, optionally, an oracle check of the results."""

    def __init__(self, name, seed=0):
        self.name = name
        self.rng = np.random.default_rng(90000 + seed)
        self.gated = []          # (live, stage, poison)
        self.outs = []           # (key, live, result)
        self.keep = []
        self.call = None         # call(stream): stream a c_void_p, or None for the null stream
        self.oracle_check = None  # oracle_check(res): res(key) -> numpy array of the result
        self.after = None        # after(): host-side checks once the stream is idle (pinned host memory)
        self.before = None       # before(): host-side reset before a run

    def live(self, a, b=None, out=None, pad=0, pad_value=None):
        """A live device tensor that is gated: `a` is copied into it behind the gate, it holds `b` (default: junk) before.
        out = key: the tensor is read back after the entry.  pad > 0: the image gets `pad` more pixels per row (a pitched image);
        the caller takes the view [:, :W] of what comes back, the padding keeps pad_value on both sides."""
        a = np.ascontiguousarray(a)
        b = junk_like(self.rng, a) if b is None else np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (self.name, a.shape, b.shape, a.dtype, b.dtype)
        if pad:
            def widen(x):
                fill = pad_value if pad_value is not None else (-7 if x.dtype == np.int32 else np.nan)
                wide = np.full((x.shape[0], x.shape[1] + pad) + x.shape[2:], fill, dtype=x.dtype)
                wide[:, :x.shape[1]] = x
                return wide
            a, b = widen(a), widen(b)
        live, stage, poison = dev(b).clone(), dev(a), dev(b)
        self.gated.append((live, stage, poison))
        if out is not None:
            self.outs.append((out, live, torch.empty_like(live)))
        return live

    def state_image(self, shape, dtype, out, start=None, pad=0):
        """A state or output image: starts from `start` (default zeros), holds junk before the gate opens, is read back."""
        a = np.zeros(shape, dtype) if start is None else np.full(shape, start, dtype)
        return self.live(a, out=out, pad=pad)

    # ---- the steps of a run
    def poison(self):
        for live, _, poison in self.gated:
            live.copy_(poison)

    def load(self, non_blocking=False):
        for live, stage, _ in self.gated:
            live.copy_(stage, non_blocking=non_blocking)

    def read_back(self):
        for _, live, result in self.outs:
            result.copy_(live, non_blocking=True)

    def snapshot(self):
        return [bits(result).copy() for _, _, result in self.outs]

    def res(self, key):
        for k, _, result in self.outs:
            if k == key:
                return result.cpu().numpy()
        raise KeyError(key)


def run_on_null_stream(case):
    """f(A): the entry on the null stream with A resident.  Also the enqueue time of the row."""
    for warm in (False, True):       # the first pass sizes workspaces and caches tables, like the gated run's warm-up: the second is timed
        if case.before:
            case.before()
        case.poison()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        case.load(non_blocking=True)
        case.call(None)
        case.read_back()
        ENQUEUE_US[case.name] = (time.perf_counter() - t0) * 1e6
        torch.cuda.synchronize()
        if case.after:
            case.after()
    return case.snapshot()


def run_gated(api, case, side, gate, warm_up=True):
    """The gated sequence of the module docstring on `side`; returns the results' bits."""
    case.poison()
    torch.cuda.synchronize()
    if warm_up:                  # sizes the per-stream workspaces, caches tables, sets kernel attributes
        case.call(side.handle)
        side.synchronize()
        case.poison()
        torch.cuda.synchronize()
    if case.before:
        case.before()
    assert torch.cuda.current_stream().cuda_stream == 0
    t0 = time.perf_counter()
    gate.close(api, side)
    with torch.cuda.stream(side.ext):
        case.load(non_blocking=True)
    case.call(side.handle)
    with torch.cuda.stream(side.ext):
        case.read_back()
    closed = gate.closed()
    enqueue_us = (time.perf_counter() - t0) * 1e6
    side.synchronize()
    GATE_TICKS.append(gate.ticks())
    GATED_US[case.name] = enqueue_us
    assert closed, ("%s: the gate had opened before the last call was enqueued (enqueue took %.0f us, the gate lasted %.0f us): "
                    "the row proves nothing" % (case.name, enqueue_us, gate.ticks() / 100.0))
    if case.after:
        case.after()
    return case.snapshot()


def assert_same_bits(case, got, want, what):
    for (key, _, _), g, w in zip(case.outs, got, want):
        assert g.shape == w.shape
        assert np.array_equal(g, w), "%s, %s: image %r differs in %d of %d elements" % (case.name, what, key, int((g != w).sum()), g.size)


@contextlib.contextmanager
def settings(api, spec_kw=None, parts=None, split=None, path=None):
    """Per-device host-side switches an entry reads when it is called."""
    try:
        if spec_kw:
            api.set_filter_spec(**spec_kw)
        if parts is not None:
            api.force_filter_parts(parts)
        if split is not None:
            api.set_filter_split(split)
        if path is not None:
            api.accumulate_records_interleaved_path(path)
        yield
    finally:
        if spec_kw:
            api.set_filter_spec()
        if parts is not None or split is not None:
            api.set_filter_split(0)
        if path is not None:
            api.accumulate_records_interleaved_path(api.RECORDS_PATH_AUTO)


# ================================================================ accumulation rows
def gated_states(case, W, H, types):
    """One set of gated state images per stat type (start: no samples), plus the epilogue's mean_corr / discriminator."""
    sts = []
    for i, (_, c, transform, _, _) in enumerate(types):
        st = {"n": case.state_image((H, W), np.int32, out=("n", i))}
        for k in ("mean", "m2", "m3"):
            st[k] = case.state_image((H, W, c), np.float32, out=(k, i))
        for k in ("film_mean", "film_m2"):
            st[k] = case.state_image((H, W, c), np.float32, out=(k, i)) if transform else None
        sts.append(st)
    mc = case.state_image((H, W, 3), np.float32, out="mean_corr", start=7.0)
    dc = case.state_image((H, W, 3), np.float32, out="discriminator", start=7.0)
    return sts, (mc, dc)


def oracle_on_records(case, oracle, W, H, types, counts, pixels, samples):
    """test_records_gpu.assert_matches_the_oracle on the case's results."""
    st = [{k: torch.from_numpy(case.res((k, i))) for k in ("n", "mean", "m2", "m3", "film_mean", "film_m2")
           if not (k.startswith("film") and not t[2])} for i, t in enumerate(types)]
    for s, t in zip(st, types):
        if not t[2]:
            s["film_mean"] = s["film_m2"] = None
    S = pytypes.SimpleNamespace(W=W, H=H, types=types, st=st)
    assert_matches_the_oracle(oracle, S, counts, pixels, samples)


def dense_samples(rng, S, W, H, types, half):
    out = []
    for i, s in enumerate(make_samples(rng, S * W * H, types)):
        s = s.reshape(S, H, W, -1)
        if half[i]:
            s = np.minimum(s, np.float32(60000.0)).astype(np.float16)
        out.append(np.ascontiguousarray(s))
    return out


def tile_tables(W, H, S, ts=16):
    """16 x 16 tiles, ragged right and bottom; samples per tile cycle through S, 0 (untouched), 3, S - 1."""
    bounds, per_tile = [], []
    for k, (y0, x0) in enumerate((y, x) for y in range(0, H, ts) for x in range(0, W, ts)):
        bounds.append((x0, y0, min(x0 + ts, W), min(y0 + ts, H)))
        per_tile.append((S, 0, 3, S - 1)[k % 4])
    bounds, per_tile = np.array(bounds, np.int32), np.array(per_tile, np.int32)
    px = (bounds[:, 2] - bounds[:, 0]) * (bounds[:, 3] - bounds[:, 1])
    sizes = (px * per_tile).astype(np.int64)
    return bounds, (np.cumsum(sizes) - sizes).astype(np.int64), per_tile


def tile_arena(smp, bounds, per_tile):
    blocks = [smp[:per_tile[k], y0:y1, x0:x1].reshape(-1) for k, (x0, y0, x1, y1) in enumerate(bounds)]
    return np.ascontiguousarray(np.concatenate(blocks + [np.zeros(8, smp.dtype)]))


def accumulate_case(api, oracle, name, W, H, kind, offset=False, S=7, types=TYPES):
    """statmc_accumulate and its film-major and tile-fed relatives.  Every variant is a dense [S][H][W][C] sample array per
    type and a per-pixel count of how many of its samples are live, which is what the oracle check is given."""
    case = Case(name, seed=W + len(name))
    rng_a, rng_b = np.random.default_rng(500 + W), np.random.default_rng(600 + W)
    half = [("formats" in kind) and t[0] in ("normal", "depth") for t in types]
    smp_a, smp_b = dense_samples(rng_a, S, W, H, types, half), dense_samples(rng_b, S, W, H, types, half)
    sts, pre = gated_states(case, W, H, types)
    formats = [api.SAMPLES_F16 if h else api.SAMPLES_F32 for h in half] if "formats" in kind else None
    cnt = np.full((H, W), S, np.int64)
    rows = counts_live = None
    tiles = kind.startswith("tiles")
    if kind == "row_ranges":
        rows = [(0, H // 3), (H // 2, H)]
        cnt[H // 3:H // 2] = 0
    if kind == "rows":              # one range: statmc_accumulate_rows
        rows = (H // 3, H)
        cnt[:H // 3] = 0
    if "counted" in kind:           # ragged counts, some outside [0, S]: the entry clamps them
        raw_a = rng_a.integers(-2, S + 3, (H, W)).astype(np.int32)
        raw_b = rng_b.integers(-2, S + 3, (H, W)).astype(np.int32)
        lead = 1 if offset else 0   # offset: the counts image starts 4 bytes into its allocation -- the element path
        flat = lambda r: np.concatenate([np.zeros(lead, np.int32), r.reshape(-1), np.zeros(4, np.int32)])
        counts_live = case.live(flat(raw_a), flat(raw_b))[lead:lead + W * H]
        cnt = np.clip(raw_a, 0, S).astype(np.int64)
    if tiles:
        bounds, offsets, per_tile = tile_tables(W, H, S)
        for k, (x0, y0, x1, y1) in enumerate(bounds):
            cnt[y0:y1, x0:x1] = np.minimum(cnt[y0:y1, x0:x1], per_tile[k])
        d_bounds, d_offsets, d_per_tile = dev(bounds), dev(offsets), dev(per_tile)        # resident, never gated
        arenas = [case.live(tile_arena(a, bounds, per_tile), tile_arena(b, bounds, per_tile)) for a, b in zip(smp_a, smp_b)]
        stat = [api.make_stat_type_arena(arenas[i], t[1], sts[i], t[2], t[3], prepass_into=pre if t[4] else None) for i, t in enumerate(types)]

        def call(stream):
            api.accumulate_tiles(W, H, stat, d_bounds, d_offsets, d_per_tile, stream=stream, sample_formats=formats, sample_counts=counts_live)
    else:
        arenas = [case.live(a, b) for a, b in zip(smp_a, smp_b)]
        stat = [api.make_stat_type(arenas[i], sts[i], t[2], t[3], prepass_into=pre if t[4] else None) for i, t in enumerate(types)]

        def call(stream):
            api.accumulate(W, H, stat, stream=stream, rows=rows, sample_formats=formats, sample_counts=counts_live)
    case.call = call
    case.counted_path = (2 if offset or (W * H) % 4 else 1) if "counted" in kind else 0

    def check(res):
        npx = W * H
        s_idx = np.repeat(np.arange(S), npx)
        p_idx = np.tile(np.arange(npx, dtype=np.int32), S)
        pixels = np.where(s_idx < cnt.reshape(-1)[p_idx], p_idx, -1).astype(np.int32)
        oracle_on_records(case, oracle, W, H, types, cnt.reshape(-1), pixels, [a.astype(np.float32).reshape(S * npx, -1) for a in smp_a])
    case.oracle_check = check
    return case


def records_case(api, oracle, name, W, H, kind, types=TYPES, split_above=None, path=None, scale=1, seed=0):
    """The records family on the ragged counts of test_records_gpu.py (one pixel at 300 records, about 5 % dead ones)."""
    case = Case(name, seed=W + len(name) + seed)
    rng_a, rng_b = np.random.default_rng(1000 + W + seed), np.random.default_rng(2000 + W + seed)
    npx = W * H
    counts = ragged_counts(rng_a, npx) * scale
    pixels_a = records_of_counts(rng_a, counts, dead=0.05)
    n = pixels_a.size
    pixels_b = rng_b.integers(0, npx, n).astype(np.int32)            # the poison stays inside the film
    smp_a, smp_b = make_samples(rng_a, n, types), make_samples(rng_b, n, types)
    sts, pre = gated_states(case, W, H, types)
    if kind == "arrays":
        d_px = case.live(pixels_a, pixels_b)
        d_s = [case.live(a, b) for a, b in zip(smp_a, smp_b)]
        stat = [api.make_stat_type_records(d_s[i], t[1], sts[i], t[2], t[3], prepass_into=pre if t[4] else None) for i, t in enumerate(types)]

        def call(stream):
            api.accumulate_records(W, H, stat, d_px, stream=stream, split_above=split_above)
    else:
        rec_a, layout = api.pack_records(pixels_a, smp_a)
        rec_b, layout_b = api.pack_records(pixels_b, smp_b)
        assert layout.stride == layout_b.stride
        d_rec = case.live(rec_a, rec_b)
        stat = [api.make_stat_type_record_field(t[1], sts[i], t[2], t[3], prepass_into=pre if t[4] else None) for i, t in enumerate(types)]

        def call(stream):
            with settings(api, path=path):
                api.accumulate_records_interleaved(W, H, stat, d_rec, layout, stream=stream, split_above=split_above)
            if path is not None:
                assert api.last_accumulate_records_interleaved_path() == path
    case.call = call
    if split_above is None:
        case.oracle_check = lambda res: oracle_on_records(case, oracle, W, H, types, counts, pixels_a, smp_a)
    else:
        assert (counts > split_above).sum() == 1                     # one pixel above split_above: bits of the null-stream run only
    return case


# ================================================================ combine rows
def combine_case(api, name, many):
    """7 x 3: own-count entries with film images of their own and one entry that borrows entry 0's counts.  K = 5 parts for
    statmc_combine_many: 9 own-count entries + 1 = 19 chains, more than the 16 one launch holds -- several launches."""
    W, H = 7, 3
    case = Case(name, seed=7 + many)
    rng = np.random.default_rng(31 + many)
    n_own, n_src = (9, 4) if many else (2, 1)

    def side(i, k, transform, with_n, out):
        st = {}
        if with_n:
            n = rng.integers(0, 40, (H, W)).astype(np.int32)
            n[0, :3] = 0                                             # nB == 0 / nA == 0 pixels
            st["n"] = case.live(n, out=("n", i, k) if out else None)
        for f in ("mean", "m2", "m3") + (("film_mean", "film_m2") if transform else ()):
            st[f] = case.live(rng.normal(0, 1, (H, W, 3)).astype(np.float32), out=(f, i, k) if out else None)
        return st
    entries = []
    for i in range(n_own + 1):
        own = i < n_own
        dst = side(i, 0, own, own, True)
        srcs = [side(i, 1 + k, own, own, False) for k in range(n_src)]
        mm, count_of = (3, -1) if own else (1, 0)
        entries.append(api.make_combine_many_entry(dst, srcs, 3, mm, count_of=count_of) if many else
                       api.make_combine_entry(dst, srcs[0], 3, mm, count_of=count_of))
    if many:
        case.call = lambda stream: api.combine_many(W, H, entries, stream=stream)
    else:
        case.call = lambda stream: api.combine_statistics(W, H, entries, stream=stream)
    return case


# ================================================================ filter rows
@functools.lru_cache(maxsize=None)
def film_statistics(W, H, seed):
    """Oracle-accumulated statistics of a small synthetic film (conftest.make_case), shared by the filter rows."""
    _, _, st = make_case(W, H, 8, seed=seed)
    rad = st["radiance"]
    return dict(n=rad["n"], mean=rad["mean"], m2=rad["m2"], m3=rad["m3"], film=rad["film_mean"], g0=st["normal"]["mean"], g1=st["albedo"]["mean"])


def filter_inputs(oracle, W, H, seed, spec_kw=None):
    d = dict(film_statistics(W, H, seed))
    spec = oracle.FilterSpec(**spec_kw) if spec_kw else None
    d["mc"], d["disc"] = oracle.prepass(d["n"], d["mean"], d["m2"], d["m3"], spec=spec)
    return d


def window_case(api, oracle, name, W=300, H=41, radius=RADIUS, sd=FILTER_SD, spec_kw=None, parts=None, split=None, floats=0, pitch=False,
                with_oracle=True, seed=0):
    """statmc_window_filter on resident pre-pass images.  floats = k: filter<float> with k one-channel buffers."""
    case = Case(name, seed=W + radius + seed)
    A, B = filter_inputs(oracle, W, H, 40 + W + seed, spec_kw), filter_inputs(oracle, W, H, 41 + W + seed, spec_kw)
    pad = (lambda k: k) if pitch else (lambda k: 0)
    view = lambda t: t[:, :W]
    welch = bool(spec_kw) and spec_kw.get("dof") == 1
    gbs = [view(case.live(A["g0"], B["g0"], pad=pad(6))), view(case.live(A["g1"], B["g1"], pad=pad(7)))]
    n = [view(case.live(A["n"], B["n"], pad=pad(3)))] if welch else []
    if floats:
        scales = [np.float32(1.0 / (1 + b // 3)) for b in range(floats)]
        pick = lambda d, k, b: np.ascontiguousarray(d[k][..., b % 3] * scales[b])
        mcs = [view(case.live(pick(A, "mc", b), pick(B, "mc", b), pad=pad(1 + b))) for b in range(floats)]
        dcs = [view(case.live(pick(A, "disc", b), pick(B, "disc", b), pad=pad(2))) for b in range(floats)]
        cols = [view(case.live(pick(A, "film", b), pick(B, "film", b), pad=pad(3))) for b in range(floats)]
        outs = [view(case.state_image((H, W), np.float32, out=("filtered", b), start=SENTINEL, pad=pad(1))) for b in range(floats)]
        n = n * floats
        channels = 1
    else:
        mcs = [view(case.live(A["mc"], B["mc"], pad=pad(2)))]
        dcs = [view(case.live(A["disc"], B["disc"], pad=pad(5)))]
        cols = [view(case.live(A["film"], B["film"], pad=pad(4)))]
        outs = [view(case.state_image((H, W, 3), np.float32, out=("filtered", 0), start=SENTINEL, pad=pad(1)))]
        channels = 3
    a, keep = api.make_filter_args(n, [], [], [], cols, mcs, dcs, outs, gbs, g_dr=G_DR, filter_sd=sd, radius=radius)
    case.keep.append(keep)
    case.variant = None

    def call(stream):
        a.stream = stream
        with settings(api, spec_kw=spec_kw, parts=parts, split=split):
            api.window_filter(a, channels)
        case.variant = api.last_filter_variant()
    case.call = call
    if with_oracle and not floats:
        def check(res):
            ospec = oracle.FilterSpec(**spec_kw) if spec_kw else None
            gb = [A["g0"], A["g1"]]
            ref = oracle.filter_image(A["mc"], A["disc"], A["film"], gb, G_DR, -0.5 / sd ** 2, radius, spec=ospec, n=A["n"] if welch else None)
            got = case.res(("filtered", 0))[:, :W]
            assert_per_pixel(oracle, got, ref, A["mc"], A["disc"], A["film"], gb, G_DR, -0.5 / sd ** 2, radius, name, spec=ospec,
                             n=A["n"] if welch else None)
        case.oracle_check = check
    return case


def whole_filter_case(api, oracle, name, channels):
    """statmc_filter_f32x3 / statmc_filter_f32: pre-pass + window filter in one entry."""
    W, H = 300, 41
    case = Case(name, seed=channels)
    A, B = filter_inputs(oracle, W, H, 340, None), filter_inputs(oracle, W, H, 341, None)
    pick = (lambda d, k: d[k]) if channels == 3 else (lambda d, k: np.ascontiguousarray(d[k][..., :1]))
    shape = (H, W, channels)
    n = case.live(A["n"], B["n"])
    ins = [case.live(pick(A, k), pick(B, k)) for k in ("mean", "m2", "m3", "film")]
    gbs = [case.live(A["g0"], B["g0"]), case.live(A["g1"], B["g1"])]
    mc, dc, ff = (case.state_image(shape, np.float32, out=k, start=SENTINEL) for k in ("mean_corr", "discriminator", "filtered"))
    a, keep = api.make_filter_args([n], [ins[0]], [ins[1]], [ins[2]], [ins[3]], [mc], [dc], [ff], gbs, g_dr=G_DR, filter_sd=FILTER_SD, radius=RADIUS)
    case.keep.append(keep)

    def call(stream):
        a.stream = stream
        (api.filter_f32x3 if channels == 3 else api.filter_f32)(a)
    case.call = call

    def check(res):                                                   # the pre-pass half, bit for bit
        mcr, dr = oracle.prepass(A["n"], pick(A, "mean"), pick(A, "m2"), pick(A, "m3"))
        assert np.array_equal(case.res("mean_corr"), mcr.reshape(shape), equal_nan=True)
        assert np.array_equal(case.res("discriminator"), dr.reshape(shape), equal_nan=True)
    case.oracle_check = check
    return case


def prepass_inputs(seed, channels, H=17, W=29):
    """test_gpu_parity.test_prepass_bit_exact's inputs: n = 0, 1, table edges, zero variance, a NaN mean."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 40, (H, W)).astype(np.int32)
    n[0, :5] = [0, 1, 2, 4097, 100000]
    mean = rng.standard_normal((H, W, channels)).astype(np.float32)
    m2 = rng.random((H, W, channels), dtype=np.float32)
    m2[1, :4] = 0.0
    m3 = rng.standard_normal((H, W, channels)).astype(np.float32)
    mean[2, 3] = np.nan
    return n, mean, m2, m3


def prepass_case(api, oracle, name, channels):
    H, W = 17, 29
    case = Case(name, seed=channels)
    A, B = prepass_inputs(12, channels), prepass_inputs(13, channels)
    n, mean, m2, m3 = (case.live(a, b) for a, b in zip(A, B))
    mc = case.state_image((H, W, channels), np.float32, out="mean_corr", start=SENTINEL)
    dc = case.state_image((H, W, channels), np.float32, out="discriminator", start=SENTINEL)
    dummy = torch.zeros(H, W, channels, device=DEV)
    a, keep = api.make_filter_args([n], [mean], [m2], [m3], [dummy], [mc], [dc], [dummy.clone()], [], g_sds=[], radius=1)
    case.keep.append(keep)

    def call(stream):
        a.stream = stream
        api.prepass(a, channels)
    case.call = call
    case.inputs_a, case.inputs_b = A, B

    def check(res):
        mcr, dr = oracle.prepass(*A)
        assert np.array_equal(case.res("mean_corr"), mcr, equal_nan=True) and np.array_equal(case.res("discriminator"), dr, equal_nan=True)
    case.oracle_check = check
    return case


def pack_case(api, oracle, name, kind):
    """statmc_pack_filter_inputs / statmc_prepass_pack / statmc_prepass_pack_rows: a 300 x 41 block into a block + halo image."""
    W, H, mx, my = 300, 41, 20, 7
    case = Case(name, seed=len(name))
    A, B = filter_inputs(oracle, W, H, 340, None), filter_inputs(oracle, W, H, 341, None)
    gbs = [case.live(A["g0"], B["g0"]), case.live(A["g1"], B["g1"])]
    film = case.live(A["film"], B["film"])
    packed = case.state_image((H + 2 * my, W + 2 * mx, 15), np.float32, out="packed", start=SENTINEL)
    zero = torch.zeros(H, W, 3, device=DEV)
    if kind == "pack":
        mc, dc = case.live(A["mc"], B["mc"]), case.live(A["disc"], B["disc"])
        a, keep = api.make_filter_args([], [], [], [], [film], [mc], [dc], [zero], gbs, g_sds=[SD_NORMAL, SD_ALBEDO], radius=RADIUS)
        rows = None
    else:
        ins = [case.live(A[k], B[k]) for k in ("n", "mean", "m2", "m3")]
        mc = case.state_image((H, W, 3), np.float32, out="mean_corr", start=SENTINEL)
        dc = case.state_image((H, W, 3), np.float32, out="discriminator", start=SENTINEL)
        a, keep = api.make_filter_args([ins[0]], [ins[1]], [ins[2]], [ins[3]], [film], [mc], [dc], [zero], gbs, g_sds=[SD_NORMAL, SD_ALBEDO],
                                       radius=RADIUS)
        rows = [(0, 5), (H - 9, H)] if kind == "rows" else None
    case.keep.append(keep)

    def call(stream):
        a.stream = stream
        if kind == "pack":
            api.pack_filter_inputs(a, packed, mx, my)
        else:
            api.prepass_pack(a, packed, mx, my, rows=rows)
    case.call = call

    def check(res):
        want = np.full((H + 2 * my, W + 2 * mx, 15), SENTINEL, np.float32)
        block = np.concatenate([A["mc"], A["disc"], A["film"], A["g0"], A["g1"]], axis=2)
        for y0, y1 in (rows or [(0, H)]):
            want[my + y0:my + y1, mx:mx + W] = block[y0:y1]
        assert np.array_equal(case.res("packed"), want, equal_nan=True)
    case.oracle_check = check
    return case


# ================================================================ pointwise rows and copies
def mean_vars_case(api, oracle, name):
    H, W = 9, 31
    case = Case(name)
    ra, rb = np.random.default_rng(8), np.random.default_rng(9)
    na, nb = (r.integers(2, 50, (H, W)).astype(np.int32) for r in (ra, rb))
    ma, mb = (r.random((H, W, 3), dtype=np.float32) for r in (ra, rb))
    n, m2 = case.live(na, nb), case.live(ma, mb)
    out = case.state_image((H, W, 3), np.float32, out="film_var", start=SENTINEL)
    case.call = lambda stream: api.calculate_mean_vars([n], [m2], [out], row_n_quirk=True, stream=stream)
    case.oracle_check = lambda res: np.testing.assert_array_equal(case.res("film_var"), oracle.mean_vars(na, ma, row_n_quirk=True))
    return case


def merge_tiles_case(api, oracle, name):
    """test_gpu_parity.test_merge_tiles_matches_oracle's tiles (41 x 27, 16 x 16 tiles, ragged right and bottom), RGB with the transform."""
    W, H, ts, channels = 41, 27, 16, 3
    case = Case(name)
    dt = oracle.TILE_PIXEL_DTYPE[channels]
    bounds = [(x0, y0, min(x0 + ts, W), min(y0 + ts, H)) for y0 in range(0, H, ts) for x0 in range(0, W, ts)]
    sizes = [(x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in bounds]
    offsets = np.cumsum(sizes) - np.array(sizes)

    def tiles(seed):
        rng = np.random.default_rng(seed)
        px = np.zeros(sum(sizes), dtype=dt)
        px["n"] = rng.integers(1, 1000, px.size)
        for k in ("mean", "m2", "m3", "film_mean", "film_m2"):
            px[k] = rng.standard_normal(px[k].shape).astype(np.float32)
        return px
    pa, pb = tiles(3), tiles(4)
    raw = case.live(pa.view(np.uint8), pb.view(np.uint8))
    st = {"n": case.state_image((H, W), np.int32, out="n", start=-7)}
    for k in ("mean", "m2", "m3", "film_mean", "film_m2"):
        st[k] = case.state_image((H, W, channels), np.float32, out=k, start=SENTINEL)
    d_bounds, d_offsets = dev(np.array(bounds, np.int32)), dev(offsets.astype(np.int64))           # resident, never gated
    case.call = lambda stream: api.merge_tiles(W, H, channels, True, raw, d_bounds, d_offsets, ts * ts, st, stream=stream)

    def check(res):
        ref = oracle.new_state(H, W, channels)
        for k in ref:
            ref[k][...] = -7
        for b, o, s in zip(bounds, offsets, sizes):
            oracle.merge_tile(pa[o:o + s].copy(), channels, *b, ref, transform=True)
        for k in ref:
            assert np.array_equal(case.res(k), ref[k]), k
    case.oracle_check = check
    return case


def tile_moments_case(api, oracle, name):
    H, W, ts = 37, 50, 16
    case = Case(name)
    va, vb = (np.random.default_rng(s).lognormal(0, 1, (H, W, 3)).astype(np.float32) for s in (1, 2))
    v = case.live(va, vb)
    out = case.state_image((-(-H // ts), -(-W // ts), 3, 3), np.float32, out="moments", start=SENTINEL)
    case.call = lambda stream: api.tile_moments(v, ts, out, stream=stream)
    case.oracle_check = lambda res: np.testing.assert_array_equal(case.res("moments"), oracle.tile_moments(va, ts))
    return case


def film_update_case(api, oracle, name):
    n = 1000
    case = Case(name)

    def pixels(seed):
        rng = np.random.default_rng(seed)
        px = np.zeros(n, dtype=oracle.FILM_PIXEL_DTYPE)
        px["xyz"] = rng.random((n, 3)) * 4
        px["filter_weight_sum"] = rng.integers(0, 5, n)
        px["splat_xyz"] = rng.random((n, 3)) * (rng.random((n, 1)) < 0.1)
        px["pad"] = np.nan
        return px
    pa, pb = pixels(17), pixels(18)
    raw = case.live(pa.view(np.uint8), pb.view(np.uint8))
    out = case.state_image((n, 3), np.float32, out="film", start=SENTINEL)
    case.call = lambda stream: api.film_update(raw, n, out, splat_scale=0.25, scale=1.5, stream=stream)
    case.oracle_check = lambda res: np.testing.assert_array_equal(case.res("film"), oracle.film_update(pa, splat_scale=0.25, scale=1.5))
    return case


def copy_rect_case(api, name):
    """A 9 x 5 rectangle of 12-byte pixels from (3, 2) of one image to (1, 4) of another, same device."""
    case = Case(name)
    rng = np.random.default_rng(5)
    src = case.live(rng.random((11, 17, 3), dtype=np.float32))
    dst = case.live(rng.random((13, 15, 3), dtype=np.float32), out="dst")
    s_img, d_img = api.image_of(src), api.image_of(dst)
    lib = api.load()
    case.call = lambda stream: api.check(lib.statmc_copy_rect(C.byref(d_img), 0, 1, 4, C.byref(s_img), 0, 3, 2, 9, 5, 12, stream))
    return case


def memory_case(api, name):
    """statmc_upload / statmc_download on pinned host memory (statmc_malloc_host) and statmc_memset.  The upload's and the
    memset's targets are overwritten by a gated copy first, the download's source is filled by one: each lands only behind it."""
    nbytes = 4096
    case = Case(name)
    lib = api.load()
    rng = np.random.default_rng(77)
    host = [C.c_void_p(), C.c_void_p()]
    for h in host:
        api.check(lib.statmc_malloc_host(C.byref(h), nbytes))
    src = np.ctypeslib.as_array(C.cast(host[0], C.POINTER(C.c_uint8)), (nbytes,))
    back = np.ctypeslib.as_array(C.cast(host[1], C.POINTER(C.c_uint8)), (nbytes,))
    payload = rng.integers(0, 256, nbytes).astype(np.uint8)
    src[:] = payload
    up = case.live(rng.integers(0, 256, nbytes).astype(np.uint8), out="uploaded")
    down_a = rng.integers(0, 256, nbytes).astype(np.uint8)
    down = case.live(down_a)
    ms = case.live(rng.integers(0, 256, nbytes).astype(np.uint8), out="memset")

    def call(stream):
        api.check(lib.statmc_upload(up.data_ptr(), host[0], nbytes, stream))
        api.check(lib.statmc_download(host[1], down.data_ptr(), nbytes, stream))
        api.check(lib.statmc_memset(ms.data_ptr(), 0x5A, nbytes, stream))
    case.call = call

    def before():
        back[:] = 0

    def after():
        assert np.array_equal(back, down_a), "statmc_download: %d of %d bytes are not the gated source's" % (int((back != down_a).sum()), nbytes)
        assert np.array_equal(case.res("uploaded"), payload) and (case.res("memset") == 0x5A).all()
    case.before, case.after = before, after
    case.free = lambda: [api.check(lib.statmc_free_host(h)) for h in host]
    return case


# ================================================================ the table
def film_id(f):
    return "%dx%d" % f


TABLE = {}
for _film in ((37, 29), (64, 32)):
    for _kind in ("plain", "row_ranges", "formats"):
        TABLE["accumulate_%s-%s" % (_kind, film_id(_film))] = functools.partial(accumulate_case, W=_film[0], H=_film[1], kind=_kind)
    for _kind, _off in (("counted", False), ("tiles_counted", False)):
        TABLE["accumulate_%s-%s" % (_kind, film_id(_film))] = functools.partial(accumulate_case, W=_film[0], H=_film[1], kind=_kind, offset=_off)
for _kind in ("rows", "tiles", "tiles_formats"):
    TABLE["accumulate_%s-37x29" % _kind] = functools.partial(accumulate_case, W=37, H=29, kind=_kind)
for _kind in ("counted", "tiles_counted"):      # the element path from a counts image 4 bytes off its allocation
    TABLE["accumulate_%s_offset-64x32" % _kind] = functools.partial(accumulate_case, W=64, H=32, kind=_kind, offset=True)
TABLE.update({
    "records-37x29": functools.partial(records_case, W=37, H=29, kind="arrays"),
    "records_interleaved_fused-37x29": lambda api, oracle, name: records_case(api, oracle, name, 37, 29, "interleaved", types=TYPES[:3], path=2),
    "records_interleaved_per_type-37x29": lambda api, oracle, name: records_case(api, oracle, name, 37, 29, "interleaved", path=1),
    "records_split-37x29": functools.partial(records_case, W=37, H=29, kind="arrays", split_above=256),
    "records_interleaved_split-37x29": functools.partial(records_case, W=37, H=29, kind="interleaved", split_above=256),
    "combine_statistics-7x3": lambda api, oracle, name: combine_case(api, name, False),
    "combine_many-7x3-K5": lambda api, oracle, name: combine_case(api, name, True),
    "prepass-1ch": functools.partial(prepass_case, channels=1),
    "prepass-3ch": functools.partial(prepass_case, channels=3),
    "window_filter-sym_r20-parts3": functools.partial(window_case, parts=3),
    "window_filter-sym_r20_clamp": functools.partial(window_case, spec_kw=dict(border=1)),
    "window_filter-sym_welch": functools.partial(window_case, spec_kw=dict(dof=1)),
    "window_filter-float5": functools.partial(window_case, floats=5, split=1),
    "window_filter-generic-r24": functools.partial(window_case, W=45, H=33, radius=24, sd=12.0),
    "window_filter-pitched": functools.partial(window_case, W=68, H=25, pitch=True),
    "filter_f32x3": functools.partial(whole_filter_case, channels=3),
    "filter_f32": functools.partial(whole_filter_case, channels=1),
    "pack_filter_inputs": functools.partial(pack_case, kind="pack"),
    "prepass_pack": functools.partial(pack_case, kind="prepass_pack"),
    "prepass_pack_rows": functools.partial(pack_case, kind="rows"),
    "calculate_mean_vars": mean_vars_case,
    "merge_tiles": merge_tiles_case,
    "tile_moments": tile_moments_case,
    "film_update": film_update_case,
    "copy_rect": lambda api, oracle, name: copy_rect_case(api, name),
    "memset_upload_download": lambda api, oracle, name: memory_case(api, name),
})
EXPECTED_VARIANT = {"window_filter-sym_r20-parts3": "sym_r20", "window_filter-sym_r20_clamp": "sym_r20_clamp", "window_filter-sym_welch": "sym_welch",
                    "window_filter-float5": "sym_r20_f+lds_r20_f", "window_filter-generic-r24": "generic", "window_filter-pitched": "sym_r20"}


@pytest.fixture(scope="module")
def side(gpu):
    """The side stream of the gated rows, and its gate."""
    assert torch.cuda.current_stream().cuda_stream == 0, "the harness races the side stream against the null stream"
    s, gate = stream_apart_from_the_null_stream(gpu)
    yield s, gate
    s.destroy()


@pytest.mark.parametrize("row", list(TABLE))
def test_entry_runs_on_its_stream(gpu, oracle, side, row):
    api = gpu
    s, gate = side
    case = TABLE[row](api, oracle, name=row)
    try:
        want = run_on_null_stream(case)
        if row in EXPECTED_VARIANT:
            assert case.variant == EXPECTED_VARIANT[row], case.variant
        if getattr(case, "counted_path", 0):
            assert api.last_accumulate_counted() == case.counted_path
        got = run_gated(api, case, s, gate)
        assert_same_bits(case, got, want, "gated on the side stream against the null-stream run")
        if case.oracle_check:
            case.oracle_check(case.res)
    finally:
        if hasattr(case, "free"):
            torch.cuda.synchronize()
            case.free()


def test_cold_window_filter_behind_the_gate(gpu, oracle):
    """A window filter at an (r, sd) no other test uses, gated on a stream that has run no entry yet, with no warm-up: its
    spatial table is uploaded synchronously inside the call, and the result must not depend on the gate for that."""
    api = gpu
    s, gate = stream_apart_from_the_null_stream(api, candidates=(None, 1))     # (with the module's stream: three alive at most)
    try:
        case = window_case(api, oracle, "window_filter-cold-r11", radius=11, sd=5.37)
        got = run_gated(api, case, s, gate, warm_up=False)
        assert case.variant == "sym_rt", case.variant
        want = run_on_null_stream(case)
        assert_same_bits(case, got, want, "cold and gated against the null-stream run afterwards")
        run_gated(api, case, s, gate, warm_up=False)          # (the results the oracle check reads: the gated ones)
        case.oracle_check(case.res)
    finally:
        s.destroy()


# ================================================================ controls
def test_control_prepass_on_the_null_stream_reads_the_poison(gpu, oracle, side):
    """statmc_prepass enqueued on the NULL stream while its inputs are gated on s: it runs while the gate is closed and returns
    f(B), which is not f(A).  The harness would have caught a wholly misplaced call."""
    api = gpu
    s, gate = side
    case = prepass_case(api, oracle, "control-prepass", 3)
    f_a = run_on_null_stream(case)
    for live, stage, poison in case.gated[:4]:                 # f(B): B resident (the outputs start from their sentinel)
        stage_b = poison
        live.copy_(stage_b)
    for live, stage, _ in case.gated[4:]:
        live.copy_(stage)
    case.call(None)
    case.read_back()
    torch.cuda.synchronize()
    f_b = case.snapshot()
    assert any(not np.array_equal(x, y) for x, y in zip(f_a, f_b))
    case.poison()
    for live, stage, _ in case.gated[4:]:
        live.copy_(stage)
    torch.cuda.synchronize()
    gate.close(api, s)
    with torch.cuda.stream(s.ext):
        case.load(non_blocking=True)
    case.call(None)                                            # misplaced: the null stream
    case.read_back()                                           # ... and read back there, before the gate opens
    torch.cuda.current_stream().synchronize()
    closed = gate.closed()
    s.synchronize()
    assert closed, "the gate had opened before the null stream was idle: the control proves nothing"
    assert_same_bits(case, case.snapshot(), f_b, "misplaced on the null stream: f(B)")


def test_control_accumulate_on_the_null_stream_is_overwritten(gpu, oracle, side):
    """statmc_accumulate enqueued on the NULL stream while samples and state are gated on s: it folds B into junk early, and the
    late copy of the start state overwrites what it wrote -- the state comes out as the start state, bit for bit."""
    api = gpu
    s, gate = side
    case = accumulate_case(api, oracle, "control-accumulate", 37, 29, "plain")
    f_a = run_on_null_stream(case)
    case.poison()
    torch.cuda.synchronize()
    gate.close(api, s)
    with torch.cuda.stream(s.ext):
        case.load(non_blocking=True)
    case.call(None)                                            # misplaced: the null stream
    with torch.cuda.stream(s.ext):
        case.read_back()
    torch.cuda.current_stream().synchronize()
    closed = gate.closed()
    s.synchronize()
    assert closed, "the gate had opened before the null stream was idle: the control proves nothing"
    start = []
    for key, live, _ in case.outs:
        stage = next(st for lv, st, _ in case.gated if lv is live)
        start.append(bits(stage))
    got = case.snapshot()
    assert_same_bits(case, got, start, "misplaced on the null stream: the start state")
    assert any(not np.array_equal(x, y) for x, y in zip(got, f_a))


# ================================================================ halo exchange
def test_halo_exchange_with_both_blocks_gated(gpu, side):
    """statmc_halo_exchange on a 2 x 1 grid of blocks on one device, each block on a side stream of its own, both gated: every
    copy runs on its destination block's stream behind the source block's event.  Against the ungated exchange."""
    from statmc_amd.peer import Block
    api = gpu
    lib = api.load()
    s0, gate0 = side
    s1, gate1 = SideStream(api), Gate()
    try:
        bw, bh, r, ch = 24, 9, 5, 15
        rng = np.random.default_rng(3)
        cases = [Case("halo-block%d" % b, seed=b) for b in range(2)]
        packed = [c.live(rng.random((bh, bw + r, ch), dtype=np.float32), out="packed") for c in cases]
        blocks = (Block * 2)()
        for b in range(2):
            blocks[b].device = 0
            blocks[b].packed = api.image_of(packed[b])

        def exchange(streams):
            for b in range(2):
                blocks[b].stream = streams[b]
            api.check(lib.statmc_halo_exchange(blocks, 2, 1, bw, bh, r))
        for c in cases:
            c.load()
        torch.cuda.synchronize()
        exchange([None, None])
        for c in cases:
            c.read_back()
        torch.cuda.synchronize()
        want = [c.snapshot() for c in cases]
        a0, a1 = (c.gated[0][1].cpu().numpy() for c in cases)
        assert np.array_equal(want[0][0].view(np.float32)[:, bw:], a1[:, r:2 * r]) and np.array_equal(want[1][0].view(np.float32)[:, :r], a0[:, bw - r:bw])
        for c in cases:
            c.poison()
        torch.cuda.synchronize()
        exchange([s0.handle, s1.handle])                      # warm-up (peer bookkeeping)
        s0.synchronize()
        s1.synchronize()
        for c in cases:
            c.poison()
        torch.cuda.synchronize()
        gate0.close(api, s0)
        gate1.close(api, s1)
        for c, s in zip(cases, (s0, s1)):
            with torch.cuda.stream(s.ext):
                c.load(non_blocking=True)
        exchange([s0.handle, s1.handle])
        for c, s in zip(cases, (s0, s1)):
            with torch.cuda.stream(s.ext):
                c.read_back()
        closed = gate0.closed() and gate1.closed()
        s0.synchronize()
        s1.synchronize()
        assert closed, "a gate had opened before the exchange was enqueued: the test proves nothing"
        for c, w in zip(cases, want):
            assert_same_bits(c, c.snapshot(), w, "both blocks gated against the ungated exchange")
    finally:
        s1.destroy()


# ================================================================ concurrency and lifetime
def run_solo(case, s):
    """The case on stream s with A resident, nothing gated; returns the results' bits."""
    case.load()
    torch.cuda.synchronize()
    case.call(s.handle)
    with torch.cuda.stream(s.ext):
        case.read_back()
    s.synchronize()
    return case.snapshot()


PAIRS = {
    "records+interleaved": (functools.partial(records_case, W=37, H=29, kind="arrays"), functools.partial(records_case, W=64, H=32, kind="interleaved")),
    "records_split+interleaved_split": (functools.partial(records_case, W=37, H=29, kind="arrays", split_above=256),
                                        functools.partial(records_case, W=64, H=32, kind="interleaved", split_above=256)),
    "welch+clamp": (functools.partial(window_case, spec_kw=dict(dof=1), with_oracle=False),
                    functools.partial(window_case, W=280, H=26, spec_kw=dict(border=1), with_oracle=False)),
    "float5+pitched": (functools.partial(window_case, floats=5, split=1), functools.partial(window_case, W=68, H=25, pitch=True, with_oracle=False)),
}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_streams_released_together(gpu, oracle, side, pair):
    """PROBABILISTIC (module docstring).  s1 and s2 wait (statmc_stream_wait_event) on an event recorded behind one gate on a
    third stream, so both start in the same instant; the two entries work on films of different sizes, so their per-stream
    workspaces differ in size.  Each result equals its own solo run on the same stream, bit for bit: scratch keyed by device
    only -- one workspace for both -- would let one call's partial sums or sorted records reach the other's result."""
    api = gpu
    lib = api.load()
    s0, gate = side
    streams = [SideStream(api), SideStream(api)]
    event = C.c_void_p()
    api.check(lib.statmc_event_create(C.byref(event)))
    try:
        cases = [make(api, oracle, name="%s-%d" % (pair, i)) for i, make in enumerate(PAIRS[pair])]
        solo = [run_solo(c, s) for c, s in zip(cases, streams)]            # (also sizes the workspaces)
        for c in cases:
            c.load()
        torch.cuda.synchronize()
        gate.close(api, s0)
        api.check(lib.statmc_event_record(event, s0.handle))
        for c, s in zip(cases, streams):
            api.check(lib.statmc_stream_wait_event(s.handle, event))
        for c, s in zip(cases, streams):
            c.call(s.handle)
        for c, s in zip(cases, streams):
            with torch.cuda.stream(s.ext):
                c.read_back()
        closed = gate.closed()
        for s in [s0] + streams:
            s.synchronize()
        assert closed, "the gate had opened before both calls were enqueued: the streams did not start together"
        for c, w in zip(cases, solo):
            assert_same_bits(c, c.snapshot(), w, "released together with the other stream's call, against its solo run")
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_event_destroy(event))
        for s in streams:
            s.destroy()


def test_records_workspace_grows_and_is_reused_on_one_stream(gpu, oracle, side):
    """Ungated, one side stream: records calls with few, many and few records again.  The per-(device, stream) workspace grows
    for the second call and is reused by the third; all three results are the null-stream run's bits."""
    api = gpu
    s, _ = side
    for k, (W, H, scale) in enumerate(((37, 29, 1), (64, 32, 12), (37, 29, 1))):
        for kind in ("arrays", "interleaved"):
            case = records_case(api, oracle, "growth-%d-%s" % (k, kind), W, H, kind, scale=scale, seed=k)
            want = run_on_null_stream(case)
            case.poison()
            assert_same_bits(case, run_solo(case, s), want, "on the side stream against the null-stream run")


def test_stream_lifetime(gpu, oracle):
    """A stream's scratch goes with statmc_stream_destroy.  A stream created afterwards may get the same handle: larger calls on
    it must not find the destroyed stream's smaller workspaces.  Another stream created and destroyed while the first one's calls
    are in flight takes nothing of the first one's with it."""
    api = gpu

    def cases(big, tag):
        W, H = ((64, 32) if big else (37, 29))
        fw, fh = ((300, 41) if big else (68, 25))
        return [records_case(api, oracle, "lifetime-records-" + tag, W, H, "arrays", scale=6 if big else 1),
                window_case(api, oracle, "lifetime-filter-" + tag, W=fw, H=fh, parts=3, with_oracle=False),
                window_case(api, oracle, "lifetime-pitched-" + tag, W=fw, H=fh, pitch=True, with_oracle=False)]
    first = SideStream(api)
    small = cases(False, "small")
    want_small = [run_on_null_stream(c) for c in small]
    for c, w in zip(small, want_small):
        c.poison()
        assert_same_bits(c, run_solo(c, first), w, "on the first stream")
    first.destroy()
    second = SideStream(api)                                    # may be the same handle
    try:
        large = cases(True, "large")
        want_large = [run_on_null_stream(c) for c in large]
        for c in large + small[:1]:
            c.load()
        torch.cuda.synchronize()
        for c in large:
            c.call(second.handle)
        other = SideStream(api)                                 # comes and goes while `second` is busy
        try:
            small[0].call(other.handle)
            with torch.cuda.stream(other.ext):
                small[0].read_back()
            other.synchronize()
            got_other = small[0].snapshot()
        finally:
            other.destroy()
        with torch.cuda.stream(second.ext):
            for c in large:
                c.read_back()
        second.synchronize()
        assert_same_bits(small[0], got_other, want_small[0], "on the stream in between")
        for c, w in zip(large, want_large):
            assert_same_bits(c, c.snapshot(), w, "larger calls on the stream created after the destroy")
        for c, w in zip(large, want_large):                     # ... and once more, now that the other stream is gone
            c.poison()
            assert_same_bits(c, run_solo(c, second), w, "after the stream in between was destroyed")
    finally:
        second.destroy()


def test_enqueue_times_and_gate_length():
    """Prints what the module docstring records: the host time to enqueue every row on the null stream and how long the gates
    lasted.  Runs after the table (a run of this test alone has nothing to report and passes)."""
    if not ENQUEUE_US or not GATE_TICKS:
        return
    print("\nstreams set aside because they shared the null stream's hardware queue: %d %s" % (len(SET_ASIDE), SET_ASIDE))
    slowest = max(ENQUEUE_US, key=ENQUEUE_US.get)
    shortest_gate_us = min(GATE_TICKS) / 100.0
    print()
    for name, us in sorted(ENQUEUE_US.items(), key=lambda kv: -kv[1]):
        print("enqueue %-44s %6.0f us on the null stream%s" % (name, us, ", %6.0f us behind the gate (gate launches included)" % GATED_US[name] if name in GATED_US else ""))
    print("gate: %d x %d shader clocks, shortest %.0f us, longest %.0f us; slowest row %s %.0f us; ratio %.1f" % (
        GATE_PROBES, PROBE_CYCLES, shortest_gate_us, max(GATE_TICKS) / 100.0, slowest, ENQUEUE_US[slowest], shortest_gate_us / ENQUEUE_US[slowest]))
