"""numpy float32 restatement of statmc_upsample_filtered (include/statmc.h), for tests/test_upsample_cpu.py (its own properties)
and tests/test_upsample_gpu.py (the device's bits).  The gate's and the feature distance's fmaf come from libm through ctypes; the
weights and the sums are ordinary float32 operations, each rounded once; a float64 evaluation of the same taps stands beside them."""
import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
GATE_SYMMETRIC, GATE_ASYMMETRIC, GATE_CENTRE = 0, 1, 2
CHANNELS_AND, CHANNELS_JOINT = 0, 1
BORDER_CLIP, BORDER_CLAMP = 0, 1
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))     # (j, i): the order of the sums

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_fmaf = np.frompyfunc(lambda a, b, c: _libm.fmaf(a, b, c), 3, 1)


def fmaf(a, b, c):
    """libm's fmaf, element by element over float32 arrays: one rounding."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        return _fmaf(a, b, c).astype(F32).reshape(a.shape)


def fmaf_fast(a, b, c):
    """The same values for films too large to walk element by element (tools/time_upsample.py): a * b is exact in float64, so
    a * b + c there has ONE rounding, and rounding that to float32 equals fmaf's single rounding unless the float64 sum sits exactly
    half-way between two float32 neighbours (its low 29 bits are 0x10000000) or the result is below the float32 normal range, where
    the half-way points lie elsewhere.  Those elements, and only those, go to libm."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        wide = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = wide.astype(F32)
        unsure = np.isfinite(wide) & (((wide.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(wide) < 2.0 ** -125))
    if unsure.any():
        out = out.copy()
        out[unsure] = fmaf(a[unsure], b[unsure], c[unsure])
    return out


def coarse_size(w, h, k):
    return (w + k - 1) // k, (h + k - 1) // k


def grid_position(n, k):
    """Per fine coordinate 0 .. n - 1: (X0, weight of X0, weight of X0 + 1).  Python's // and % are the floor and its remainder."""
    x = np.arange(n, dtype=np.int64)
    t = 2 * x + 1 - k
    x0 = t // (2 * k)
    a = t - 2 * k * x0
    assert ((a % 2 == 1) & (a >= 1) & (a <= 2 * k - 1)).all()
    w0 = (2 * k - a).astype(F32) / F32(2 * k)
    w1 = a.astype(F32) / F32(2 * k)
    assert (w0.astype(np.float64) + w1.astype(np.float64) == 1.0).all()      # dyadic: exact
    return x0, w0, w1


def pixel_valid(mc, disc, colour, g):
    """the oracle's pixel_valid: [H, W] bool"""
    v = np.isfinite(mc).all(-1) & ~np.isnan(disc).any(-1) & np.isfinite(colour).all(-1)
    for G in g:
        v &= np.isfinite(G).all(-1)
    return v


def pair_member(gate, rule, mc_p, d_p, mc_q, d_q, fma=fmaf):
    """the oracle's pair_member under per-pixel dof, over [..., C] arrays: [...] bool"""
    with np.errstate(all="ignore"):
        d = (mc_p - mc_q).astype(F32)
        if gate == GATE_CENTRE:
            lhs, rhs = (d * d).astype(F32), d_p
        elif gate == GATE_ASYMMETRIC:
            lhs, rhs = fma(d, d, -d_q), d_p
        else:
            lhs, rhs = fma(d, d, -((d_p + d_q).astype(F32))), np.zeros_like(d_p)
        ok = (lhs <= rhs).all(-1)
        ls, rs = lhs[..., 0], rhs[..., 0]
        for c in range(1, lhs.shape[-1]):
            ls, rs = (ls + lhs[..., c]).astype(F32), (rs + rhs[..., c]).astype(F32)
    return (ls <= rs) if rule == CHANNELS_JOINT else ok


def _img(a):
    a = np.asarray(a, F32)
    return a[..., None] if a.ndim == 2 else a


def upsample_ref(fine, coarse, k, gate=0, rule=0, border=0, g_dr=(), fma=fmaf):
    """fine: dict(mean_corr, disc, colour, g=[...]) of [H, W(, C)] float32 arrays; coarse: dict(mean_corr, disc, filtered, g=[...]) of
    [Hc, Wc(, C)].  Returns dict(out [H, W, C] float32, out64 [H, W, C] float64 -- the same taps, weights and sums in double --,
    member [H, W, 4] bool -- the taps that entered the sums, in TAPS order --, fallback [H, W] bool -- the pixels that pass their own
    colour through).  fma: fmaf (libm, element by element) or fmaf_fast (the same values, vectorised)."""
    mc, disc, col = _img(fine["mean_corr"]), _img(fine["disc"]), _img(fine["colour"])
    cmc, cdisc, cf = _img(coarse["mean_corr"]), _img(coarse["disc"]), _img(coarse["filtered"])
    fg, cg = [_img(G) for G in fine.get("g", [])], [_img(G) for G in coarse.get("g", [])]
    h, w, ch = mc.shape
    wc, hc = coarse_size(w, h, k)
    assert cmc.shape == (hc, wc, ch) and len(fg) == len(cg) == len(g_dr)
    x0, wx0, wx1 = grid_position(w, k)
    y0, wy0, wy1 = grid_position(h, k)
    wx, wy = (wx0, wx1), (wy0, wy1)
    p_valid = pixel_valid(mc, disc, col, fg)
    q_valid = pixel_valid(cmc, cdisc, cf, cg)
    sum_w = np.zeros((h, w), F32)
    acc = np.zeros((h, w, ch), F32)
    sum64 = np.zeros((h, w), np.float64)
    acc64 = np.zeros((h, w, ch), np.float64)
    member = np.zeros((h, w, 4), bool)
    with np.errstate(all="ignore"):
        for tap, (j, i) in enumerate(TAPS):
            X, Y = x0 + i, y0 + j
            inside = ((Y >= 0) & (Y < hc))[:, None] & ((X >= 0) & (X < wc))[None, :]
            Xc, Yc = np.clip(X, 0, wc - 1), np.clip(Y, 0, hc - 1)
            take = p_valid & (inside if border == BORDER_CLIP else True)
            iy, ix = Yc[:, None], Xc[None, :]
            take = take & q_valid[iy, ix]
            take = take & pair_member(gate, rule, mc, disc, cmc[iy, ix], cdisc[iy, ix], fma)
            e = np.zeros((h, w), F32)
            e64 = np.zeros((h, w), np.float64)
            for G, Gc, dr in zip(fg, cg, g_dr):
                d = (G - Gc[iy, ix]).astype(F32)
                dist2 = (d[..., 0] * d[..., 0]).astype(F32)
                for c in range(1, d.shape[-1]):
                    dist2 = fma(d[..., c], d[..., c], dist2)
                e = fma(F32(dr), dist2, e)
                d64 = G.astype(np.float64) - Gc[iy, ix].astype(np.float64)
                e64 = e64 + np.float64(F32(dr)) * (d64 * d64).sum(-1)
            tent = (wy[j][:, None] * wx[i][None, :]).astype(F32)
            wgt = (tent * np.exp(e).astype(F32)).astype(F32)
            wgt64 = tent.astype(np.float64) * np.exp(e64)
            q_col = cf[iy, ix]
            sum_w = np.where(take, (sum_w + wgt).astype(F32), sum_w)
            term = (wgt[..., None] * q_col).astype(F32)
            acc = np.where(take[..., None], (acc + term).astype(F32), acc)
            sum64 = np.where(take, sum64 + wgt64, sum64)
            acc64 = np.where(take[..., None], acc64 + wgt64[..., None] * q_col.astype(np.float64), acc64)
            member[..., tap] = take
        some = sum_w > 0
        out = np.where(some[..., None], (acc / np.where(some, sum_w, F32(1))[..., None]).astype(F32), col)
        out64 = np.where(some[..., None], acc64 / np.where(some, sum64, 1.0)[..., None], col.astype(np.float64))
    # the pass-through is a copy of bits (a NaN colour keeps its payload)
    out = out.astype(F32)
    out.view(np.uint32)[~some] = col.view(np.uint32)[~some]
    return dict(out=out, out64=out64, member=member, fallback=~some, sum64=sum64)
