"""numpy restatement of statmc_score_window (include/statmc.h), for tests/test_score_window_cpu.py (its own properties) and
tests/test_score_window_gpu.py (the device's bits).  The keys are tests/select_reference.py's.  Two forms: window_brute visits
every tap of every pixel and is for small images; window_ref is separable -- the maximum over 2 r + 1 shifted copies along x, then
along y, on an image padded with the identity -- and fast enough for 1280 x 720.  Neither doubles nor tiles as the device does."""
import numpy as np

import select_reference as sel

F32 = np.float32
MAX, MIN = 0, 1
MAX_RADIUS = 32
IDENTITY = {MAX: np.uint32(0), MIN: np.uint32(0xFFFFFFFF)}      # of a tap outside the film


def keys_image(score):
    """uint32 keys [H, W] of a float32 image [H, W]"""
    score = np.asarray(score, F32)
    return sel.keys_of(score).reshape(score.shape)


def as_float(keys):
    return np.ascontiguousarray(keys, np.uint32).view(F32)


def window_brute(score, op, radius):
    """out[y][x] over the pixels (x', y') of the film with |x' - x| <= radius and |y' - y| <= radius: pixel by pixel, the whole
    clipped square of each"""
    k = keys_image(score)
    h, w = k.shape
    out = np.empty((h, w), np.uint32)
    for y in range(h):
        for x in range(w):
            square = k[max(0, y - radius):min(h, y + radius + 1), max(0, x - radius):min(w, x + radius + 1)]
            out[y, x] = square.max() if op == MAX else square.min()
    return as_float(out)


def window_ref(score, op, radius):
    """the same, separably: shifted copies of the identity-padded key image along x, then along y"""
    assert op in (MAX, MIN) and 0 <= radius <= MAX_RADIUS
    k = keys_image(score)
    h, w = k.shape
    fold = np.maximum if op == MAX else np.minimum
    p = np.full((h, w + 2 * radius), IDENTITY[op], np.uint32)
    p[:, radius:radius + w] = k
    rows = p[:, 0:w].copy()
    for d in range(1, 2 * radius + 1):
        rows = fold(rows, p[:, d:d + w])
    p = np.full((h + 2 * radius, w), IDENTITY[op], np.uint32)
    p[radius:radius + h] = rows
    out = p[0:h].copy()
    for d in range(1, 2 * radius + 1):
        out = fold(out, p[d:d + h])
    return as_float(out)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


# ---------------------------------------------------------------- the images both test files use
IMAGES = ["lognormal", "mixed_classes", "constant", "ramp", "ramp_mirror"]


def image(name, w, h):
    """float32 [h, w].  lognormal: every pixel another value.  mixed_classes: NaN of both signs, negatives, -0, -inf, +inf,
    subnormals and the class borders 2^-60 / 2^60 with the patterns next to them, among lognormal values.  ramp / ramp_mirror:
    x + y and its mirror -- the answer is a corner of the window, so a window one short or one long on either side shows."""
    import plan_reference as plan_ref
    rng = np.random.default_rng(w * 1000 + h + IMAGES.index(name))
    px = w * h
    if name == "lognormal":
        return plan_ref.lognormal_scores(h, w, seed=w + 7)
    if name == "constant":
        return np.full((h, w), 0.75, F32)
    if name in ("ramp", "ramp_mirror"):
        y, x = np.mgrid[0:h, 0:w]
        r = (x + y).astype(F32) + F32(1)
        return r if name == "ramp" else (F32(w + h) - r).astype(F32)
    if name == "mixed_classes":
        b = bits(plan_ref.lognormal_scores(h, w, seed=w + 9)).reshape(-1).copy()
        special = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xC0600000, 0x80000000, 0xFF800000, 0x7F800000, 0x00000001, 0x000002CA, 0x80000001,
                            sel.LIVE_LO, sel.LIVE_LO - 1, sel.LIVE_LO + 1, sel.LIVE_HI, sel.LIVE_HI - 1, sel.LIVE_HI + 1, 0x00000000], np.uint32)
        kinds = rng.integers(0, 3 * len(special), px)
        hit = kinds < len(special)
        b[hit] = special[kinds[hit]]
        return b.view(F32).reshape(h, w)
    raise KeyError(name)


def impulse_sites(w, h):
    """the corners, the middle of every edge and the centre"""
    xs, ys = sorted({0, w // 2, w - 1}), sorted({0, h // 2, h - 1})
    return [(x, y) for y in ys for x in xs]


def impulse(w, h, site, op):
    """MAX: one large value in a film of small ones; MIN: one zero in a constant film"""
    s = np.full((h, w), 0.5 if op == MAX else 2.0, F32)
    s[site[1], site[0]] = F32(1e6) if op == MAX else F32(0)
    return s


def impulse_answer(w, h, site, op, radius):
    """exactly the clipped square around the site"""
    s = np.full((h, w), 0.5 if op == MAX else 2.0, F32)
    x, y = site
    s[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = F32(1e6) if op == MAX else F32(0)
    return s
