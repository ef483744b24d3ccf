"""numpy float32 restatement of statmc_sample_scores and statmc_plan_samples (include/statmc.h), for tests/test_plan_cpu.py (its own
properties) and tests/test_plan_gpu.py (the device's bits).  T(u) is found by bisection over the uint32 bit patterns of the level --
not by the device's 64-way passes."""
import numpy as np

F32 = np.float32
U_LO, U_HI = 0x20000000, 0x5F000000
LIVE_LO, LIVE_HI = F32(2.0 ** -60), F32(2.0 ** 60)
MAX_TARGET = 1 << 30
MAX_COUNT = 1 << 20
ABSOLUTE, RELATIVE = 0, 1


def scores_ref(n, film_mean, film_m2, metric, eps):
    """n int32 [H, W]; film_mean, film_m2 float32 [H, W, C]; every numpy float32 operation rounds once, division and square root
    correctly."""
    n = np.asarray(n, np.int32)
    mean = np.asarray(film_mean, F32).reshape(n.shape + (-1,))
    m2 = np.asarray(film_m2, F32).reshape(n.shape + (-1,))
    with np.errstate(all="ignore"):
        fn = (n.astype(np.int64) - 1).astype(F32)
        v = m2[..., 0] / fn
        for c in range(1, m2.shape[-1]):
            v = v + m2[..., c] / fn
        sd = np.sqrt(v)
        assert sd.dtype == F32
        if metric == RELATIVE:
            a = np.abs(mean[..., 0])
            for c in range(1, mean.shape[-1]):
                a = a + np.abs(mean[..., c])
            sd = sd / (F32(eps) + a)
    assert sd.dtype == F32
    return np.where(n < 2, F32(np.inf), sd).astype(F32)


def classes(score):
    s = np.asarray(score, F32)
    with np.errstate(invalid="ignore"):
        sat = s > LIVE_HI
        live = (s >= LIVE_LO) & (s <= LIVE_HI)
    return live, sat


def level_of(u):
    return np.array([u], np.uint32).view(F32)[0]


def counts_at(u, score, n, c_min, c_max):
    """c_p(u) for every pixel, int64"""
    s = np.asarray(score, F32)
    live, sat = classes(s)
    nn = np.zeros(s.shape, np.int64) if n is None else np.clip(np.asarray(n, np.int64), 0, MAX_TARGET)
    t = (level_of(u) * np.where(live, s, F32(1))).astype(F32)
    big = t >= F32(MAX_TARGET)
    N = np.where(big, MAX_TARGET, np.ceil(np.where(big, F32(0), t)).astype(np.int64))
    c = np.clip(N - nn, c_min, c_max)
    return np.where(live, c, np.where(sat, c_max, c_min)).astype(np.int64)


def total_at(u, score, n, c_min, c_max):
    return int(counts_at(u, score, n, c_min, c_max).sum())


def plan_ref(score, n, budget, c_min, c_max):
    """(sample_counts int32 like score, result dict with the fields of statmc_plan_result)"""
    score = np.asarray(score, F32)
    live, sat = classes(score)
    res = dict(budget=int(budget), n_live=int(live.sum()), n_saturated=int(sat.sum()))
    T = lambda u: total_at(u, score, n, c_min, c_max)
    if budget <= T(U_LO):
        c = counts_at(U_LO, score, n, c_min, c_max)
        res.update(status=1, level_bits=U_LO, total=int(c.sum()))
        return c.astype(np.int32), res
    if budget > T(U_HI):
        c = counts_at(U_HI, score, n, c_min, c_max)
        res.update(status=2, level_bits=U_HI, total=int(c.sum()))
        return c.astype(np.int32), res
    lo, hi = U_LO, U_HI          # T(lo) < budget <= T(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if T(mid) >= budget:
            hi = mid
        else:
            lo = mid
    base = counts_at(hi - 1, score, n, c_min, c_max)
    d = counts_at(hi, score, n, c_min, c_max) - base
    R = budget - int(base.sum())
    flat = d.reshape(-1)
    E = np.concatenate([[0], np.cumsum(flat)[:-1]]).reshape(d.shape)
    c = base + np.clip(R - E, 0, d)
    res.update(status=0, level_bits=hi, total=int(c.sum()))
    return c.astype(np.int32), res


def lognormal_scores(h, w, seed, sigma=1.5):
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.0, sigma, (h, w))).astype(F32)
