"""Device-side film statistics + the accumulate -> pre-pass -> window-filter pass, expressed
with the reference's buffer names (t<type>-b<bounce>-{n,mean,m2,m3,film-mean,film-m2,mean-corr,
discriminator,film-mean-f}, "film", "film-f"; estimator.cpp:101-161).  Holds torch tensors only
as HBM allocations; all arithmetic happens in libstatmc_hip.so.
"""
import torch

from . import api

# (channels, transform, max_moment, filter sd) of the shipped denoise configuration
# (statpath.cpp:1027-1160; scenes/render-denoise.pbrt:19-22) plus the two float G-buffers (their sds: this build's
# choice for the synthetic scene -- the reference takes them from the scene file's `filterbuffersds`, no default).
STAT_TYPES = {
    "radiance":   dict(channels=3, transform=True,  max_moment=3, sd=None),
    "normal":     dict(channels=3, transform=False, max_moment=1, sd=0.1),
    "albedo":     dict(channels=3, transform=False, max_moment=1, sd=0.02),
    "depth":      dict(channels=1, transform=False, max_moment=1, sd=1.0),
    "materialid": dict(channels=1, transform=False, max_moment=1, sd=0.5),
}


def new_state(height, width, channels, device, transform=True, placed=False):
    """placed: the images come from statmc_malloc_placed(STATMC_MEM_STATE) -- one HBM rank, apart from the sample arenas
    (api.empty_placed(..., api.MEM_STREAM)): include/statmc.h, "Device memory placed by HBM rank"."""
    if placed:
        z = lambda: api.zeros_placed((height, width, channels), torch.float32, device, api.MEM_STATE)
        n = api.zeros_placed((height, width), torch.int32, device, api.MEM_STATE)
    else:
        z = lambda: torch.zeros(height, width, channels, dtype=torch.float32, device=device)
        n = torch.zeros(height, width, dtype=torch.int32, device=device)
    st = dict(n=n, mean=z(), m2=z(), m3=z())
    if transform:
        st["film_mean"], st["film_m2"] = z(), z()
    else:  # non-transform types alias mean/m2 (estimator.cpp:127-137)
        st["film_mean"], st["film_m2"] = None, None
    return st


class FilmStats:
    """One GPU's block of the film: per-type running moments and the filter's work images."""

    def __init__(self, width, height, device, types=("radiance", "normal", "albedo"),
                 filter_sd=10.0, radius=20, g_buffers=("normal", "albedo"), g_sds=None, placed=False, fused_prepass=False):
        """fused_prepass: whole-film accumulations also write the radiance type's mean-corr / discriminator in their epilogue
        (statmc_stat_type::mean_corr / discriminator: the bits of statmc_prepass), and prepass() has nothing left to do while
        that result is current -- same filter spec and significance level, no row-range accumulation, no reset since."""
        api.setup(device.index if device.index is not None else 0)
        self.width, self.height, self.device = width, height, device
        self.types = list(types)
        self.placed = placed
        self.state = {t: new_state(height, width, STAT_TYPES[t]["channels"], device,
                                   STAT_TYPES[t]["transform"], placed=placed) for t in self.types}
        self.filter_sd, self.radius = filter_sd, radius
        self.g_names = list(g_buffers)
        self.g_sds = list(g_sds) if g_sds is not None else [STAT_TYPES[g]["sd"] for g in self.g_names]
        # the filter's work images are written by one kernel and read by the next: with the moments (placed: state role)
        z3 = (lambda: api.zeros_placed((height, width, 3), torch.float32, device, api.MEM_STATE)) if placed else \
             (lambda: torch.zeros(height, width, 3, dtype=torch.float32, device=device))
        self.mean_corr, self.disc, self.film, self.film_f = z3(), z3(), z3(), z3()
        self.fused_prepass = bool(fused_prepass)
        self._prepass_current = None      # (filter spec, significance) under which the epilogue's result was written
        self._previews = {}               # k -> the coarse film of preview(k), kept for the next call at that k

    def reset(self):
        self._prepass_current = None
        for st in self.state.values():
            for v in st.values():
                if v is not None:
                    v.zero_()

    def accumulate(self, samples, rows=None, counts=None):
        """samples: {type: [S, H, W, C]}; one kernel launch covers every stat type.  rows = (y0, y1): only those rows.
        A type's arena is read in the format of its tensor: torch.float32, or torch.float16 (statmc_accumulate_formats: the bits
        of the same samples widened to fp32).  counts: int32 CUDA tensor [H, W] -- pixel p folds only its first
        min(max(counts[p], 0), S) samples and keeps every bit where that is 0 (statmc_accumulate_counted): the arena of a
        renderer that spends its samples unevenly."""
        if counts is not None and tuple(counts.shape) != (self.height, self.width):
            raise ValueError("FilmStats.accumulate: counts must be [H, W] = [%d, %d]" % (self.height, self.width))
        fuse = self.fused_prepass and rows is None and "radiance" in samples
        sts = [api.make_stat_type(samples[t], self.state[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"],
                                  prepass_into=(self.mean_corr, self.disc) if (fuse and t == "radiance") else None)
               for t in self.types if t in samples]
        fmts = []
        for t in self.types:
            if t in samples:
                if samples[t].dtype not in (torch.float32, torch.float16):
                    raise TypeError("FilmStats.accumulate: samples of %r are %s; torch.float32 or torch.float16" % (t, samples[t].dtype))
                fmts.append(api.SAMPLES_F16 if samples[t].dtype == torch.float16 else api.SAMPLES_F32)
        # (an all-fp32 batch makes the call it always made)
        api.accumulate(self.width, self.height, sts, rows=rows, sample_formats=fmts if api.SAMPLES_F16 in fmts else None, sample_counts=counts)
        if counts is not None and fuse:
            # pixels without a live sample keep their mean-corr / discriminator: current only if they were current before
            key = self._prepass_key()
            self._prepass_current = key if self._prepass_current == key else None
        else:
            self._prepass_current = self._prepass_key() if fuse else None

    def accumulate_compact(self, samples=None, offsets=None, n_samples=None, split_above=None, records=None, layout=None):
        """samples: {type: [n_samples, C]} compact arenas -- every pixel's samples back to back, pixels in raster order -- in
        torch.float32 or torch.float16; offsets: int64 CUDA tensor [H * W + 1] (api.compact_offsets of the count image): pixel p
        folds positions [offsets[p], offsets[p + 1]) in ascending order and keeps every bit where that run is empty
        (statmc_compact_accumulate: the bits of statmc_accumulate_records on the same samples).  n_samples: the arenas' length in
        samples, None = the shortest tensor's; split_above: None = api.RECORDS_SPLIT_DEFAULT.
        records=, layout= instead of samples: the same arena as ONE array of interleaved records (uint8 or int32 CUDA tensor; the
        record of pixel p's sample s at slot offsets[p] + s) -- layout = (stride, {type: byte offset | (byte offset, api.SAMPLES_F32 |
        api.SAMPLES_F16)}); n_samples counts records then (statmc_compact_accumulate_interleaved: the bits of the call on the
        de-interleaved arenas)."""
        if offsets is None or (samples is None) == (records is None) or (records is None) != (layout is None):
            raise ValueError("FilmStats.accumulate_compact: offsets with either samples, or records and layout")
        if records is not None:
            stride, fields = layout
            fuse = self.fused_prepass and "radiance" in fields
            names = [t for t in self.types if t in fields]
            sts = [api.make_stat_type_record_field(STAT_TYPES[t]["channels"], self.state[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"],
                                                   prepass_into=(self.mean_corr, self.disc) if (fuse and t == "radiance") else None) for t in names]
            at = [fields[t] if isinstance(fields[t], (tuple, list)) else (fields[t], api.SAMPLES_F32) for t in names]
            lay = api.make_record_layout(stride, 0, [o for o, _ in at], [f for _, f in at])
            api.compact_accumulate_interleaved(self.width, self.height, sts, records, lay, offsets, n_records=n_samples, split_above=split_above)
            key = self._prepass_key()
            self._prepass_current = key if (fuse and self._prepass_current == key) else None
            return
        fuse = self.fused_prepass and "radiance" in samples
        sts, fmts = [], []
        for t in self.types:
            if t not in samples:
                continue
            if samples[t].dtype not in (torch.float32, torch.float16):
                raise TypeError("FilmStats.accumulate_compact: samples of %r are %s; torch.float32 or torch.float16" % (t, samples[t].dtype))
            sts.append(api.make_stat_type_compact(samples[t], STAT_TYPES[t]["channels"], self.state[t], STAT_TYPES[t]["transform"],
                                                  STAT_TYPES[t]["max_moment"], prepass_into=(self.mean_corr, self.disc) if (fuse and t == "radiance") else None))
            fmts.append(api.SAMPLES_F16 if samples[t].dtype == torch.float16 else api.SAMPLES_F32)
        api.compact_accumulate(self.width, self.height, sts, offsets, n_samples=n_samples,
                               sample_formats=fmts if api.SAMPLES_F16 in fmts else None, split_above=split_above)
        # pixels with an empty run keep their mean-corr / discriminator: current only if they were current before
        key = self._prepass_key()
        self._prepass_current = key if (fuse and self._prepass_current == key) else None

    def _state_types(self, prepass):
        fuse = prepass and self.fused_prepass and "radiance" in self.types
        return [api.make_stat_type_record_field(STAT_TYPES[t]["channels"], self.state[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"],
                                                prepass_into=(self.mean_corr, self.disc) if (fuse and t == "radiance") else None)
                for t in self.types], fuse

    def gather_states(self, pixels):
        """The states of the listed pixels as records: pixels is an int32 CUDA tensor of y * width + x (a value outside the film:
        the state of no samples).  Returns {type: int32 tensor [n, D]} (statmc_gather_states); the film is only read.  The list of
        the pixels a plan touches is api.compact_offsets(counts, cap=1, owners_capacity=...)[1]."""
        sts, _ = self._state_types(False)
        return dict(zip(self.types, api.gather_states(self.width, self.height, sts, pixels)))

    def combine_records(self, pixels, states, split_above=None):
        """Merges (pixel, state) records -- gather_states of another film of the same types, or records a renderer's kernel wrote
        with PixelStats::write_record -- into this film: per pixel in ascending record index, the bits of combine_ with the same
        parts in that order; a pixel without a record of positive count keeps every bit (statmc_combine_records).  states: {type:
        int32 tensor [n, D]} for every type of this film.  split_above: None = never split.  With fused_prepass the touched pixels'
        mean-corr / discriminator are written by the launch's epilogue."""
        if set(states) != set(self.types):
            raise ValueError("combine_records: states must carry this film's stat types (%s / %s)" % (self.types, sorted(states)))
        sts, fuse = self._state_types(True)
        api.combine_records(self.width, self.height, sts, pixels, [states[t] for t in self.types], split_above=split_above)
        # pixels without a record keep their mean-corr / discriminator: current only if they were current before
        key = self._prepass_key()
        self._prepass_current = key if (fuse and self._prepass_current == key) else None

    def combine_(self, other):
        """Combines the statistics of `other` -- the same film, its own samples -- into self, so that self holds the
        statistics of the union of both sample sets (statmc_combine_statistics: one launch).  Every stat type is weighed
        with its own counts; the colour image `film` with the radiance counts.  With fused_prepass the launch's epilogue
        writes mean-corr / discriminator of the combined radiance moments (the bits of statmc_prepass).

        `other` may also be a sequence of films: they are folded into self in that order by statmc_combine_many -- the bits
        of one combine_ per film, every part read once and self written once (groups of api.MAX_COMBINE_SOURCES)."""
        many = not isinstance(other, FilmStats)
        others = list(other) if many else [other]
        for o in others:
            if (o.width, o.height) != (self.width, self.height) or o.device != self.device:
                raise ValueError("combine_: both films must have the same size and device")
            if set(o.types) != set(self.types):
                raise ValueError("combine_: both films must carry the same stat types (%s / %s)" % (self.types, o.types))
        fuse = self.fused_prepass and "radiance" in self.types
        with_film = "radiance" in self.types and self.film is not None and all(o.film is not None for o in others)
        for g in range(0, len(others), api.MAX_COMBINE_SOURCES):
            group = others[g:g + api.MAX_COMBINE_SOURCES]
            make = (lambda dst, srcs, *a, **kw: api.make_combine_many_entry(dst, srcs, *a, **kw)) if many else \
                   (lambda dst, srcs, *a, **kw: api.make_combine_entry(dst, srcs[0], *a, **kw))
            entries = []
            for t in self.types:
                cfg = STAT_TYPES[t]
                entries.append(make(self.state[t], [o.state[t] for o in group], cfg["channels"], cfg["max_moment"],
                                    prepass_into=(self.mean_corr, self.disc) if (fuse and t == "radiance") else None))
            if with_film:
                owner = self.types.index("radiance")
                entries.append(make({"mean": self.film}, [{"mean": o.film} for o in group], 3, 1, count_of=owner))
            if many:
                api.combine_many(self.width, self.height, entries, n_sources=len(group))
            else:
                api.combine_statistics(self.width, self.height, entries)
        if others:
            self._prepass_current = self._prepass_key() if fuse else None

    def pooled(self, k):
        """A new FilmStats of ceil(width / k) x ceil(height / k) pixels whose every pixel holds the statistics of all samples of
        a k x k block of this film (statmc_pool_statistics: one launch; k = 2, 4 or 8; this film is only read).  Every stat
        type is pooled with its own counts, the colour image `film` with the radiance counts.  With fused_prepass the launch's
        epilogue writes mean-corr / discriminator of the pooled radiance moments, so pooled(k).denoise() works as on any film."""
        wc, hc = api.pooled_size(self.width, self.height, k)
        coarse = FilmStats(wc, hc, self.device, types=self.types, filter_sd=self.filter_sd, radius=self.radius,
                           g_buffers=self.g_names, g_sds=self.g_sds, placed=self.placed, fused_prepass=self.fused_prepass)
        self._pool_into(coarse, k)
        return coarse

    def _pool_entries(self, coarse):
        """the entries of pooled(k)'s launch into `coarse`: every stat type with its own counts, "film" with the radiance counts"""
        fuse = self.fused_prepass and "radiance" in self.types
        entries = []
        for t in self.types:
            cfg = STAT_TYPES[t]
            entries.append(api.make_pool_entry(coarse.state[t], self.state[t], cfg["channels"], cfg["max_moment"],
                                               prepass_into=(coarse.mean_corr, coarse.disc) if (fuse and t == "radiance") else None))
        if "radiance" in self.types and self.film is not None:
            entries.append(api.make_pool_entry({"mean": coarse.film}, {"mean": self.film}, 3, 1, count_of=self.types.index("radiance")))
        return entries, fuse

    def _pool_into(self, coarse, k):
        """pooled(k)'s launch into an existing coarse film of the right size and types: every plane of it is written"""
        entries, fuse = self._pool_entries(coarse)
        api.pool_statistics(self.width, self.height, k, entries)
        coarse._prepass_current = coarse._prepass_key() if fuse else None

    def upsample_from(self, coarse, k, roi=None):
        """The filtered image of `coarse` -- this film pooled k x k, denoised -- brought onto this film's filtered image by
        statmc_upsample_filtered: per fine pixel the four coarse pixels around it, weighed by a bilinear tent and the G-buffer range
        term, where they pass the filter's membership test against the fine pixel; the pixel's own colour where none does.  Needs this
        film's mean-corr / discriminator (prepass()) and the coarse film's pre-pass and window filter.  One launch; the statistics of
        both films are only read.  For a host that holds its own pyramid; preview(k) runs the whole path.  Returns film_f."""
        if (coarse.width, coarse.height) != api.pooled_size(self.width, self.height, k) or coarse.device != self.device:
            raise ValueError("upsample_from: coarse must be this film pooled by k = %d, %dx%d on %s" %
                             ((k,) + api.pooled_size(self.width, self.height, k) + (self.device,)))
        if coarse.g_names != self.g_names:
            raise ValueError("upsample_from: both films must carry the same G-buffers (%s / %s)" % (self.g_names, coarse.g_names))
        fine_args, keep_f = self.filter_args(roi=roi)
        coarse_args, keep_c = coarse.filter_args()
        api.upsample_filtered(fine_args, coarse_args, k, 3)
        return self.film_f

    def preview(self, k):
        """A film-sized denoised image at the price of a filter pass over ceil(W / k) x ceil(H / k) pixels: pooled(k), the coarse
        film's pre-pass and window filter, this film's pre-pass (nothing to do after a fused epilogue), upsample_from.  k = 2, 4 or 8.
        The coarse FilmStats stays on self and is pooled into again by the next preview at the same k; this film's statistics are only
        read.  Returns film_f -- the image denoise() writes; the last iteration of a progressive render still calls denoise()."""
        coarse = self._previews.get(k)
        if coarse is None:
            coarse = self._previews[k] = self.pooled(k)
        else:
            self._pool_into(coarse, k)
        coarse.prepass()
        coarse.window_filter()
        self.prepass()
        return self.upsample_from(coarse, k)

    def plan_samples(self, budget, c_min, c_max, metric="relative", eps=1e-3, type="radiance", return_result=False, dilate=0, error=None):
        """The per-pixel sample counts of the next accumulation: `budget` samples spent by the noise of stat type `type` as it stands
        (statmc_sample_scores over its n and raw-sample Welford planes, then statmc_plan_samples with its n as the counts so far).
        Returns an int32 tensor [H, W] that accumulate(samples, counts=) takes as it is; with return_result=True, (counts, the
        statmc_plan_result as a dict) after a synchronisation.  dilate = r > 0: the plan spends by the worst score within r pixels
        (statmc_score_window, MAX), so a pixel beside a noisy one is not starved; 0: the pointwise score as it is, no extra launch.  The
        film is only read.  error: which quantity is scored -- None: the sample standard deviation, what a budget is best spent by;
        "stderr" / "ci": the error of the mean (see score_quantiles)."""
        return api.plan_samples(self._scores(metric, eps, type, dilate, error), budget, c_min, c_max, n=self.state[type]["n"], return_result=return_result)

    def _scores(self, metric, eps, type, dilate=0, error=None):
        """the score image of stat type `type` as it stands over its n and raw-sample Welford planes -- error None: the sample standard
        deviation (statmc_sample_scores); "stderr" / "ci": the standard error of the mean / the two-sided confidence half-width at the
        device's significance level (statmc_error_scores); dilate > 0: its MAX window of that radius (statmc_score_window)"""
        st = self.state[type]
        film_mean = st["film_mean"] if st["film_mean"] is not None else st["mean"]
        film_m2 = st["film_m2"] if st["film_m2"] is not None else st["m2"]
        if error is None:
            scores = api.sample_scores(st["n"], film_mean, film_m2, metric=metric, eps=eps)
        elif error in ("stderr", "ci"):
            scores = api.error_scores(st["n"], film_mean, film_m2, metric=metric, eps=eps, table=error)
        else:
            raise ValueError("error must be None, \"stderr\" or \"ci\", not %r" % (error,))
        return api.score_window(scores, dilate, "max") if dilate else scores

    def plan_to_target(self, target, c_min, c_max, budget=None, metric="relative", eps=1e-3, type="radiance", error="ci", dilate=0,
                       return_result=False):
        """The per-pixel sample counts that bring the error of the mean of stat type `type` to `target`: statmc_error_scores ("ci": the
        two-sided confidence half-width at the device's significance level; "stderr": the standard error), its MAX window for dilate > 0,
        then statmc_plan_to_target with the type's n -- n (error / target)^2 - n per open pixel, clamped to [c_min, c_max]; c_min where
        the pixel is at the target, c_max where it cannot be judged yet.  budget: if not None and the plan's total exceeds it, the budget
        is spent instead as plan_samples spends it (the sample-deviation score of the same metric, eps and dilation).  Returns an int32
        tensor [H, W] that accumulate(samples, counts=) takes as it is; with return_result=True, (counts, the statmc_target_result as a
        dict with "by_budget" and, where the fallback ran, "budgeted": the statmc_plan_result).  One synchronisation and one 48-byte
        download when budget or return_result asks for the result, none otherwise; the film is only read."""
        if error not in ("stderr", "ci"):
            raise ValueError("plan_to_target: error must be \"stderr\" or \"ci\", not %r" % (error,))
        n = self.state[type]["n"]
        errors = self._scores(metric, eps, type, dilate, error)
        if budget is None and not return_result:
            return api.plan_to_target(errors, n, target, c_min, c_max)
        counts, res = api.plan_to_target(errors, n, target, c_min, c_max, return_result=True)
        res["by_budget"] = budget is not None and res["total"] > budget
        if res["by_budget"]:
            counts, res["budgeted"] = api.plan_samples(self._scores(metric, eps, type, dilate), budget, c_min, c_max, n=n, out=counts,
                                                       return_result=True)
        return (counts, res) if return_result else counts

    def score_quantiles(self, qs, metric="relative", eps=1e-3, type="radiance", dilate=0, error=None):
        """The q-quantiles (1 to 8 values of q in [0, 1]) of the score of stat type `type` as plan_samples computes it, by the
        nearest-rank rule: rank(q) = max(0, ceil(q P) - 1) of the P pixels' keys in ascending order (statmc_score_select).  A
        renderer's stopping rule reads the error of the mean, error="stderr" or "ci": "the 95th percentile of the relative confidence
        half-width is under 2 %".  error=None is the sample standard deviation, which converges to the pixel's sigma and does not fall
        as samples arrive: no such rule can be met on it.  Returns the values as numpy float32, one per q, after one synchronisation
        and the download of one 256-byte struct; the film is only read.  dilate: as plan_samples'."""
        import math
        from fractions import Fraction
        px = self.width * self.height
        ranks = []
        for q in qs:
            if not 0 <= q <= 1:
                raise ValueError("score_quantiles: q = %r is outside [0, 1]" % (q,))
            ranks.append(max(0, math.ceil(Fraction(float(q)) * px) - 1))     # Python integers: exact in q as the double it is (numpy scalars too)
        return api.read_select_result(api.score_select(self._scores(metric, eps, type, dilate, error), ranks))["values"]

    def score_count_above(self, thresholds, metric="relative", eps=1e-3, type="radiance", dilate=0, error=None):
        """Per threshold (1 to 8) the number of pixels whose score, as plan_samples computes it, is above it
        (statmc_score_count_above: NaN and negative scores count as 0).  "At most 1 % of the pixels are above tau."  Returns a list of
        Python integers after one synchronisation and one small download; the film is only read.  dilate, error: as score_quantiles'."""
        return [int(c) for c in api.score_count_above(self._scores(metric, eps, type, dilate, error), thresholds).cpu().numpy()]

    def score_mean(self, caps=(float("inf"),), metric="relative", eps=1e-3, type="radiance", dilate=0, error="stderr"):
        """The mean and the RMS of the score of stat type `type`, per cap (1 to 4): every pixel counts as min(score, cap), NaN and
        negative scores as 0 (statmc_score_sum: exact sums, the same bits on every run).  "The mean relative half-width is under
        1 %", "the RMS relative error is under T".  A cap of +inf is no cap: the pixels nobody can judge yet (+inf, fewer than 2
        samples) are left out of the sums and of the divisor.  The score pipeline is score_quantiles': the error of the mean
        (error="stderr" or "ci"; None: the sample standard deviation, on which no such rule can be met), then the optional window.
        Returns a dict after one synchronisation and the download of one 152-byte struct; the film is only read:
        "mean" = sum / n and "rms" = sqrt(sum_sq / n) per cap, in float64 on the host, n = n_px, or n_px - n_infinite for a cap of
        +inf (NaN where n is 0); "caps", "sum", "sum_sq", "n_clipped" per cap; "n_px", "n_zero", "n_finite", "n_infinite"."""
        import math
        r = api.read_sum_result(api.score_sum(self._scores(metric, eps, type, dilate, error), caps))
        r["mean"], r["rms"] = [], []
        for j in range(r["n_caps"]):
            n = r["n_px"] - (r["n_infinite"] if r["cap_bits"][j] == 0x7F800000 else 0)
            r["mean"].append(r["sum"][j] / n if n else float("nan"))
            r["rms"].append(math.sqrt(r["sum_sq"][j] / n) if n else float("nan"))
        return r

    def score_tiles(self, tile, cap=float("inf"), metric="relative", eps=1e-3, type="radiance", dilate=0, error="stderr",
                    planes=api.TILE_PLANES):
        """Per tile x tile block (8, 16, 32 or 64) of the film the statistics of the score of stat type `type`
        (statmc_score_tiles: exact, the same bits on every run): "sum", "sum_sq" of min(score, cap) as doubles, "mean" as a
        correctly rounded float32, "max" the block's largest score, "n_px", "n_zero", "n_infinite", "n_clipped" (above the cap).  A
        renderer that works tile by tile reads its rule per region from them: the "mean" and "max" planes are score images for
        api.score_count_above / score_select / plan_samples on the tile grid, "n_clipped" a count image for api.compact_offsets
        (cap=1: the open tiles).  cap = +inf is no cap: the pixels nobody can judge yet are left out.  The score pipeline is
        score_mean's.  Returns {name: device tensor [tiles_y, tiles_x]}; no synchronisation, nothing downloaded; the film is only
        read."""
        return api.score_tiles(self._scores(metric, eps, type, dilate, error), tile, cap, planes=planes)

    def score_tile_quantiles(self, tile, qs, metric="relative", eps=1e-3, type="radiance", dilate=0, error="stderr",
                             fields=api.TILE_QUANTILE_FIELDS):
        """Per tile x tile block (8, 16, 32 or 64) of the film the q-quantiles (1 to 4) of the score of stat type `type`, by the
        nearest-rank rule within the block (statmc_score_tile_select: exact, the same bits on every run): "the 95th percentile of
        the relative half-width in this tile is under 2 %".  `qs` are (num, den) pairs or floats in [0, 1]; all share one
        denominator on the device, so pairs are brought to their least common multiple, which must not exceed 65536.  A float goes
        through Fraction(q).limit_denominator(65536): 0.95 is 19/20, and a q that is no such fraction is replaced by the nearest
        one.  The score pipeline is score_mean's.  Returns {"value": [float32 [tiles_y, tiles_x] per q], "n_below": [int32 ...],
        "n_equal": [...]} for the fields named, device tensors; no synchronisation, nothing downloaded; the film is only read.  A
        "value" plane goes to gate_tiles as it is."""
        import math
        pairs = [api.tile_quantile_fraction(q) for q in qs]
        for num, den in pairs:
            if den < 1 or not 0 <= num <= den:
                raise ValueError("score_tile_quantiles: %d/%d is outside [0, 1]" % (num, den))
        den = 1
        for _, d in pairs:
            den = den * d // math.gcd(den, d)
        if den > api.TILE_SELECT_MAX_DEN:
            raise ValueError("score_tile_quantiles: the quantiles' common denominator %d exceeds %d" % (den, api.TILE_SELECT_MAX_DEN))
        nums = [num * (den // d) for num, d in pairs]
        return api.score_tile_select(self._scores(metric, eps, type, dilate, error), tile, nums, den, fields=fields)

    def gate_tiles(self, tile, tile_value, threshold, closed=None, images=(), out=None):
        """Close the tiles of this film whose `tile_value` (a plane of score_tile_quantiles or score_tiles) is at or under
        `threshold`, for good where `closed` (an int32 plane of the tile grid, zeros before the first call) is given, and zero the
        pixels of every tile that is not open in `images` -- a score image before plan_samples, a count image after it
        (statmc_gate_tiles).  Returns (open int32 [tiles_y, tiles_x], gated images, the statmc_gate_result as a dict) after one
        synchronisation and one 32-byte download."""
        is_open, gated, res = api.gate_tiles(self.height, self.width, tile, tile_value, threshold, closed=closed, images=images, out=out)
        return is_open, gated, api.read_gate_result(res)

    def _prepass_key(self):
        return (api.get_filter_spec().as_tuple(), api.get_significance())

    def g_buffer(self, name):
        return self.state[name]["mean"]  # film-mean == mean for non-transform types

    def filter_args(self, roi=None, colour=None, out=None, rows=None):
        """rows = (y0, y1): the call sees those rows of every image as images of their own (per-pixel stages only)."""
        rad = self.state["radiance"]
        colour = colour if colour is not None else rad["film_mean"]
        out = out if out is not None else self.film_f
        cut = (lambda t: t) if rows is None else (lambda t: t[rows[0]:rows[1]])
        args, keep = api.make_filter_args(
            n=[cut(rad["n"])], mean=[cut(rad["mean"])], m2=[cut(rad["m2"])], m3=[cut(rad["m3"])], film=[cut(colour)],
            mean_corr=[cut(self.mean_corr)], disc=[cut(self.disc)], film_filtered=[cut(out)],
            g_buffers=[cut(self.g_buffer(g)) for g in self.g_names], g_sds=self.g_sds,
            filter_sd=self.filter_sd, radius=self.radius, denoise_film=False, roi=roi)
        return args, keep

    def prepass(self):
        if self._prepass_current is not None and self._prepass_current == self._prepass_key():
            return          # the last accumulation's epilogue wrote mean-corr / discriminator already (same bits)
        self._prepass_current = None
        args, keep = self.filter_args()
        api.prepass(args, 3)

    def window_filter(self, roi=None):
        args, keep = self.filter_args(roi=roi)
        api.window_filter(args, 3)

    def denoise(self):
        """Estimator::Denoise for the RGB radiance buffer: pre-pass + window filter."""
        args, keep = self.filter_args()
        api.filter_f32x3(args)
        return self.film_f
