"""numpy restatement of the three definitions of variance-guided denoising
(include/mrt.h "variance-guided denoising"): the luminance
moments recurrence, the variance estimate (mrt_variance) and the
variance-guided A-Trous filter (mrt_denoise_variance).

The moments are evaluated in float32 with the precise build's operation order
(through the oracle's accumulate, so the precise build can be compared bit for
bit) or in float64; the estimate and the filter in float32 or float64, taps in
the kernels' order (dy outer, dx inner)."""
from __future__ import annotations

import numpy as np

from denoise_model import KERNEL, NOT_FILTERABLE, _dot, words

LUM = (0.2126, 0.7152, 0.0722)
HAT = (0.25, 0.5, 0.25)


def lum(rgb, dtype=np.float32):
    """(0.2126 r + 0.7152 g) + 0.0722 b of float32 rgb [..., 3], every operation in `dtype`."""
    T = np.dtype(dtype).type
    c = np.asarray(rgb, np.float32).astype(T)
    with np.errstate(all="ignore"):
        return ((T(np.float32(LUM[0])) * c[..., 0] + T(np.float32(LUM[1])) * c[..., 1]) +
                T(np.float32(LUM[2])) * c[..., 2]).astype(T)


def moments_records(oracle_mod, rgb):
    """Oracle ray records whose radiance is (l, l*l, 0), float32, for rgb [N, 3]."""
    l = lum(rgb, np.float32)
    rays = np.zeros(len(l), oracle_mod.RAY_DTYPE)
    with np.errstate(all="ignore"):
        rays["radiance"][:, 0] = l
        rays["radiance"][:, 1] = l * l
    return rays


def moments_accumulate32(oracle_mod, frames_rgb, moments=None, first_frame=0):
    """The float32 recurrence: frames_rgb is a sequence of [N, 3] float32 path
    radiance, frame first_frame first; returns the moments image [N, 4]."""
    for k, rgb in enumerate(frames_rgb):
        if moments is None:
            moments = np.zeros((len(rgb), 4), np.float32)
        oracle_mod.accumulate(first_frame + k, moments_records(oracle_mod, np.ascontiguousarray(rgb, np.float32)), moments)
    return moments


def moments_accumulate64(frames_rgb, first_frame=0):
    """The same recurrence, c + (stored - c) f / (f + 1), in float64 (l from the float32 radiance)."""
    m = None
    with np.errstate(all="ignore"):
        for k, rgb in enumerate(frames_rgb):
            f = first_frame + k
            l = lum(rgb, np.float64)
            c = np.stack([l, l * l, np.zeros_like(l), np.ones_like(l)], -1)
            if m is None or f == 0:
                m = c
            else:
                m = c + (m - c) * (np.float64(f) / np.float64(f + 1))
                m[..., 3] = 1.0
    return m


def _planes(guide_n, guide_p, H, W, T):
    gn = np.asarray(guide_n, np.float32).reshape(H, W, 4)
    gp = np.asarray(guide_p, np.float32).reshape(H, W, 4)
    word = words(gn)
    return word, word < NOT_FILTERABLE, gn[..., :3].astype(T), gp[..., :3].astype(T), gp[..., 3].astype(T)


def _normal_weight(D, e, T):
    D = np.fmax(T(0.0), D)   # fmaxf: 0 for a NaN product
    for _ in range(e):
        D = D * D
    return D


def variance(moments, guide_n, guide_p, params, dtype=np.float64):
    """mrt_variance: moments [H, W, 4] float32 counted (mean l, mean l^2, ., n);
    params has sigma_plane, normal_log2_power, min_frames.  Returns [H, W] of `dtype`."""
    T = np.dtype(dtype).type
    moments = np.asarray(moments)   # float32 as the kernels read it (float64 for the definition's own arithmetic)
    H, W = moments.shape[:2]
    word, filt, n, x, t = _planes(guide_n, guide_p, H, W, T)
    m1, m2, cnt = (moments[..., k].astype(T) for k in (0, 1, 3))
    e, sigma_p = int(params.normal_log2_power), T(np.float32(params.sigma_plane))
    with np.errstate(all="ignore"):
        usable = np.isfinite(m1) & np.isfinite(m2) & (cnt > 0)
        temporal = usable & (cnt >= T(params.min_frames))
        vt = np.fmax(T(0.0), m2 - m1 * m1) / (cnt - T(1.0))
        sw, s1, s2 = (np.zeros((H, W), T) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                y0, y1 = max(0, -dy), min(H, H - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                ok = filt[P] & (word[Q] == word[P]) & usable[Q]
                D = _normal_weight(_dot(n[P], n[Q]), e, T)
                dist = np.abs(_dot(n[P], x[Q] - x[P]))
                w = (D * np.exp(-(dist / (sigma_p * t[P])))) * cnt[Q]
                w = np.where(ok, w, T(0.0)).astype(T)
                sw[P] += w
                s1[P] += w * np.where(ok, m1[Q], T(0.0))
                s2[P] += w * np.where(ok, m2[Q], T(0.0))
        some = sw > 0
        d = np.where(some, sw, T(1.0))
        a1, a2 = s1 / d, s2 / d
        vs = np.where(some, np.fmax(T(0.0), a2 - a1 * a1) / np.fmax(cnt, T(1.0)), T(0.0))
        r = np.where(temporal, vt, vs)
        r = np.where(filt & np.isfinite(r) & (r >= 0), r, T(0.0))
    return r.astype(T)


def _shift3(v, T):
    """The 3x3 (1/4, 1/2, 1/4)^2 average over the taps inside the image, renormalised."""
    H, W = v.shape
    gw, gv = np.zeros((H, W), T), np.zeros((H, W), T)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            k = T(HAT[dx + 1]) * T(HAT[dy + 1])
            gw[P] += k
            gv[P] += k * v[Q]
    return gv / gw


def svgf_atrous(image, var, guide_n, guide_p, params, dtype=np.float64):
    """mrt_denoise_variance: image [H, W, 4] float32, var [H, W] float32;
    params has iterations, sigma_luminance, sigma_plane, normal_log2_power.
    Returns (out [H, W, 4], variance_out [H, W]) of `dtype` (alpha copied)."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    word, filt, n, x, t = _planes(guide_n, guide_p, H, W, T)
    c = image[..., :3].astype(T)
    v = np.asarray(var, np.float32).reshape(H, W).astype(T)
    sigma_l, sigma_p = T(np.float32(params.sigma_luminance)), T(np.float32(params.sigma_plane))
    e = int(params.normal_log2_power)
    with np.errstate(all="ignore"):
        for i in range(int(params.iterations)):
            s = 1 << i
            fin = np.isfinite(c).all(-1)
            l = ((T(np.float32(LUM[0])) * c[..., 0] + T(np.float32(LUM[1])) * c[..., 1]) + T(np.float32(LUM[2])) * c[..., 2])
            g = np.fmax(_shift3(v, T), T(0.0))
            inv_l = T(1.0) / (sigma_l * np.sqrt(g) + T(np.float32(1e-6)))
            sw, sv = np.zeros((H, W), T), np.zeros((H, W), T)
            sc = np.zeros((H, W, 3), T)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1 = max(0, -dy * s), min(H, H - dy * s)
                    x0, x1 = max(0, -dx * s), min(W, W - dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    ok = filt[P] & (word[Q] == word[P]) & fin[Q]
                    D = _normal_weight(_dot(n[P], n[Q]), e, T)
                    dist = np.abs(_dot(n[P], x[Q] - x[P]))
                    arg = dist / (sigma_p * t[P]) + np.where(fin[P], np.abs(l[Q] - l[P]) * inv_l[P], T(0.0))
                    wgt = (T(KERNEL[dx + 2]) * T(KERNEL[dy + 2])) * D * np.exp(-arg)
                    wgt = np.where(ok, wgt, T(0.0)).astype(T)
                    sw[P] += wgt
                    sc[P] += wgt[..., None] * np.where(ok[..., None], c[Q], T(0.0))
                    sv[P] += (wgt * wgt) * np.where(ok, v[Q], T(0.0))
            use = filt & (sw > 0)
            d = np.where(use, sw, T(1.0))
            c = np.where(use[..., None], sc / d[..., None], c).astype(T)
            v = np.where(use, (sv / d) / d, v).astype(T)
    out = image.astype(T)
    out[..., :3] = c
    return out, v
