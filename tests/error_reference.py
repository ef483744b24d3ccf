"""numpy float32 restatement of statmc_error_scores and statmc_plan_to_target (include/statmc.h), for tests/test_error_scores_cpu.py
(its own properties) and tests/test_error_scores_gpu.py (the device's bits)."""
import numpy as np

import plan_reference as plan

F32 = np.float32
NO_TABLE = -1
DOF_MAX = 4096
TARGET_RESULT_FIELDS = ["total", "need", "n_open", "n_capped", "n_unjudged", "n_live", "n_saturated"]


def expand_table(quantiles):
    """What statmc_set_t_quantiles leaves on the device: 4096 entries, degrees of freedom past the last given one reuse it."""
    q = np.asarray(quantiles, F32).reshape(-1)
    return np.concatenate([q, np.full(DOF_MAX - q.size, q[-1], F32)]) if q.size < DOF_MAX else q[:DOF_MAX].copy()


def error_scores_ref(n, film_mean, film_m2, metric, eps, table=None):
    """n int32 [H, W]; film_mean, film_m2 float32 [H, W, C]; table: None (the standard error) or the 4096 float32 quantiles of the
    device's table.  Every numpy float32 operation rounds once, division and square root correctly."""
    n = np.asarray(n, np.int32)
    mean = np.asarray(film_mean, F32).reshape(n.shape + (-1,))
    m2 = np.asarray(film_m2, F32).reshape(n.shape + (-1,))
    n64 = n.astype(np.int64)
    with np.errstate(all="ignore"):
        fn1 = (n64 - 1).astype(F32)
        v = m2[..., 0] / fn1
        for c in range(1, m2.shape[-1]):
            v = v + m2[..., c] / fn1
        vm = v / n64.astype(F32)
        e = np.sqrt(vm)
        assert e.dtype == F32
        if table is not None:
            t = np.asarray(table, F32)
            assert t.shape == (DOF_MAX,)
            q = t[np.clip(np.minimum(n64 - 1, DOF_MAX) - 1, 0, DOF_MAX - 1)]
            e = q * e
        if metric == plan.RELATIVE:
            a = np.abs(mean[..., 0])
            for c in range(1, mean.shape[-1]):
                a = a + np.abs(mean[..., c])
            e = e / (F32(eps) + a)
    assert e.dtype == F32
    return np.where(n < 2, F32(np.inf), e).astype(F32)


def plan_to_target_ref(error, n, target, c_min, c_max):
    """(sample_counts int32 like error, result dict with the fields of statmc_target_result)"""
    e = np.asarray(error, F32)
    target = F32(target)
    live, sat = plan.classes(e)
    nn = np.clip(np.asarray(n, np.int64), 0, plan.MAX_TARGET)
    unjudged = sat | (live & (nn < 2))
    with np.errstate(all="ignore"):
        is_open = live & (nn >= 2) & (e > target)
        eo = np.where(is_open, e, target)          # r = 1 elsewhere: nothing below depends on a pixel that is not open
        r = eo / target
        r2 = r * r
        t = r2 * nn.astype(F32)
        assert t.dtype == F32
        big = t >= F32(plan.MAX_TARGET)
        N = np.where(big, plan.MAX_TARGET, np.ceil(np.where(big, F32(0), t)).astype(np.int64))
    d = np.maximum(N - nn, 0)
    c = np.where(unjudged, c_max, c_min)
    c = np.where(is_open, np.clip(d, c_min, c_max), c).astype(np.int64)
    res = dict(total=int(c.sum()), need=int(d[is_open].sum()), n_open=int(is_open.sum()), n_capped=int((is_open & (d > c_max)).sum()),
               n_unjudged=int(unjudged.sum()), n_live=int(live.sum()), n_saturated=int(sat.sum()))
    return c.astype(np.int32), res


def iid_statistics(h, w, spp, seed, channels=3):
    """Welford statistics (n, mean, m2) of spp iid samples per pixel: a per-pixel level and relative spread (both lognormal over the
    film, the same for every spp of one seed), Gaussian noise on top.  Gaussian, not a heavy tail: the sample deviation of a handful
    of heavy-tailed samples underestimates sigma, and this generator is for the behaviour of the scores under an honest estimate."""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.normal(0.0, 1.0, (h, w, channels)))
    spread = 0.3 * np.exp(rng.normal(0.0, 0.5, (h, w, 1)))
    x = level * (1.0 + spread * rng.normal(0.0, 1.0, (spp, h, w, channels)))
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    return np.full((h, w), spp, np.int32), mean.astype(F32), m2.astype(F32)
