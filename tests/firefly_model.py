"""numpy restatement of the firefly clamp's definition (include/mrt.h "firefly
suppression"), in float32 or float64, taps in the kernel's
order (dy outer, dx inner)."""
from __future__ import annotations

import numpy as np

from denoise_model import MISS_WORD, NOT_FILTERABLE, _dot, words
from variance_model import LUM


def firefly_clamp(image, guide_n, guide_p, params, dtype=np.float64):
    """mrt_firefly_clamp: image [H, W, 4] float32, guide planes [H, W, 4]
    float32; params has radius, k, min_taps, normal_cos_min, plane_tolerance.
    Returns (out [H, W, 4] of `dtype`, cap [H, W] of `dtype` — NaN where rules
    (a)-(c) do not hold —, the decision mask [H, W] bool, l [H, W] of `dtype`).
    Pixels outside the mask are the input's, exactly."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    gn = np.asarray(guide_n, np.float32).reshape(H, W, 4)
    gp = np.asarray(guide_p, np.float32).reshape(H, W, 4)
    word = words(gn)
    filt = word < NOT_FILTERABLE
    is_light = (word >= NOT_FILTERABLE) & (word < MISS_WORD)
    n, x, t = gn[..., :3].astype(T), gp[..., :3].astype(T), gp[..., 3].astype(T)
    c = image[..., :3].astype(T)
    R = int(params.radius)
    k, cos_min, tol = (T(np.float32(v)) for v in (params.k, params.normal_cos_min, params.plane_tolerance))
    with np.errstate(all="ignore"):
        fin = np.isfinite(c).all(-1)
        l = (T(np.float32(LUM[0])) * c[..., 0] + T(np.float32(LUM[1])) * c[..., 1]) + T(np.float32(LUM[2])) * c[..., 2]
        eligible = filt & fin & (l > 0)                                  # (a)
        light = np.zeros((H, W), bool)
        N = np.zeros((H, W), np.int64)
        s1, s2 = np.zeros((H, W), T), np.zeros((H, W), T)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                y0, y1 = max(0, -dy), min(H, H - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                light[P] |= is_light[Q]                                  # (b)
                if dy == 0 and dx == 0:
                    continue
                ok = (word[Q] == word[P]) & fin[Q]                       # (c); a NaN comparison is False
                ok &= _dot(n[P], n[Q]) >= cos_min
                ok &= np.abs(_dot(n[P], x[Q] - x[P])) <= tol * t[P]
                lq = np.where(ok, l[Q], T(0.0)).astype(T)
                N[P] += ok
                s1[P] += lq
                s2[P] += lq * lq
        counted = eligible & ~light & (N >= int(params.min_taps))
        d = np.where(counted, N, 1).astype(T)
        m = s1 / d
        cap = m + k * np.sqrt(np.fmax(T(0.0), s2 / d - m * m))          # (d)
        cap = np.where(counted, cap, T(np.nan)).astype(T)
        mask = counted & (l > cap)
        scale = np.where(mask, cap / np.where(mask, l, T(1.0)), T(1.0)).astype(T)
        out = image.astype(T)
        out[..., :3] = np.where(mask[..., None], c * scale[..., None], c)
    return out, cap, mask, l.astype(T)


def undecided(l64, cap64, tol):
    """The pixels whose decision (d) is within `tol` (relative) of a tie in the float64 model."""
    with np.errstate(all="ignore"):
        return np.isfinite(cap64) & (np.abs(l64 - cap64) <= tol * np.fmax(np.abs(l64), np.abs(cap64)))
