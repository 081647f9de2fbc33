"""numpy restatement of the temporal history's two definitions (include/mrt.h
"temporal history", DESIGN.md "Temporal reprojection"): resolve, which merges
the accumulation image with a counted history, and reproject, which carries a
counted image from the previous camera's view into the current one through the
guide planes of both.  Each in float64, or in float32 with the kernels'
operation order (dot products as (a0 b0 + a1 b1) + a2 b2, taps in the order
j = 0..1 (outer), i = 0..1 (inner)).

reproject also returns a FRAGILE mask: the pixels where a rounding could change
a decision of the definition, so that two correct evaluations may differ by
more than rounding:
  |cz| <= 1e-4 |v|;
  an in-image, word-matching tap whose plane distance is within 1e-4 t_p of
  the bound, or whose normal cosine is within 1e-4 of normal_cos_min;
  fx or fy within 1e-4 of an integer AND the results of the two floor choices
  differ by more than 1e-3 relative (an identical camera puts every fx near an
  integer and is not fragile: the other tap's weight goes to 0)."""
from __future__ import annotations

import numpy as np

from denoise_model import NOT_FILTERABLE, words

EPS = 1e-4


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def resolve(image, frames, history=None, dtype=np.float64):
    """[H, W, 4] of `dtype`: the counted image of `image` (float32 [H, W, 4],
    running mean of `frames` frames) merged with the counted `history`."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    I = image[..., :3].astype(T)
    n = T(np.float32(frames))
    if history is None:
        Hc = np.zeros(image.shape[:2] + (4,), T)
    else:
        Hc = np.asarray(history, np.float32).astype(T)
    h = Hc[..., 3]
    fin = np.isfinite(image[..., :3]).all(-1)
    out = np.empty(image.shape[:2] + (4,), T)
    with np.errstate(all="ignore"):
        t = h + n
        blend = (h[..., None] * Hc[..., :3] + n * I) / np.where(t > 0, t, T(1.0))[..., None]
    none = ~(h > 0)
    keep = (h > 0) & ((n == 0) | ~fin)
    out[..., :3] = np.where(none[..., None], I, np.where(keep[..., None], Hc[..., :3], blend))
    out[..., 3] = np.where(none, n, np.where(keep, h, t))
    return out


def _gather(T, prev, word_q, n_q, x_q, word_p, n_p, x_p, t_p, live, fx, fy, x0, y0, params):
    """The taps of floor choice (x0, y0): (rgbh [H, W, 4], margin-fragile mask)."""
    H, W = word_p.shape
    tol, cmin = T(np.float32(params.plane_tolerance)), T(np.float32(params.normal_cos_min))
    hmax = T(np.float32(params.max_history))
    ax, ay = fx - x0, fy - y0
    B = np.zeros((H, W), T)
    acc = np.zeros((H, W, 4), T)
    edge = np.zeros((H, W), bool)
    pfin = np.isfinite(prev[..., :3]).all(-1)
    for j in range(2):
        for i in range(2):
            qx, qy = x0 + i, y0 + j
            inside = live & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1).astype(np.int64), np.clip(qy, 0, H - 1).astype(np.int64)
            b = (ax if i else T(1.0) - ax) * (ay if j else T(1.0) - ay)
            same = inside & (word_q[cy, cx] == word_p)
            cos = _dot(n_p, n_q[cy, cx])
            dist = np.abs(_dot(n_p, x_q[cy, cx] - x_p))
            bound = tol * t_p
            edge |= same & ((np.abs(dist - bound) <= EPS * np.abs(t_p)) | (np.abs(cos - cmin) <= EPS))
            pq = prev[cy, cx]
            ok = same & (b > 0) & (cos >= cmin) & (dist <= bound) & (pq[..., 3] > 0) & pfin[cy, cx]
            bb = np.where(ok, b, T(0.0)).astype(T)
            B += bb
            acc += bb[..., None] * np.where(ok[..., None], pq, np.float32(0.0)).astype(T)
    use = B > 0
    out = acc / np.where(use, B, T(1.0))[..., None]
    out[..., 3] = np.minimum(hmax, out[..., 3])
    use &= out[..., 3] > 0
    return np.where(use[..., None], out, T(0.0)).astype(T), edge


def reproject(prev, prev_n, prev_p, prev_cam, cur_n, cur_p, params, dtype=np.float64):
    """(history [H, W, 4] of `dtype`, fragile [H, W] bool).  prev_cam has
    origin, right, up, forward and tan_half_fov (an mrt.Camera)."""
    T = np.dtype(dtype).type
    prev = np.asarray(prev, np.float32)
    H, W = prev.shape[:2]
    prev_n, prev_p, cur_n, cur_p = (np.asarray(a, np.float32).reshape(H, W, 4) for a in (prev_n, prev_p, cur_n, cur_p))
    word_p, word_q = words(cur_n), words(prev_n)
    n_p, x_p, t_p = cur_n[..., :3].astype(T), cur_p[..., :3].astype(T), cur_p[..., 3].astype(T)
    n_q, x_q = prev_n[..., :3].astype(T), prev_p[..., :3].astype(T)
    o, right, up, fwd = (np.array(list(a), np.float32).astype(T) for a in
                         (prev_cam.origin, prev_cam.right, prev_cam.up, prev_cam.forward))
    s = T(np.float32(prev_cam.tan_half_fov))
    with np.errstate(all="ignore"):
        v = x_p - o
        cz = _dot(v, fwd)
        live = (word_p < NOT_FILTERABLE) & (cz > 0)
        czs = np.where(live, cz, T(1.0))
        U, V = _dot(v, right) / czs, _dot(v, up) / czs
        sv = s * (T(H) / T(W))
        fx = (U / s + T(1.0)) * (T(0.5) * T(W - 1))
        fy = (V / sv + T(1.0)) * (T(0.5) * T(H - 1))
        live &= (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H)
        fx, fy = np.where(live, fx, T(0.0)), np.where(live, fy, T(0.0))
        x0, y0 = np.floor(fx), np.floor(fy)
        args = (T, prev, word_q, n_q, x_q, word_p, n_p, x_p, t_p, live, fx, fy)
        out, edge = _gather(*args, x0, y0, params)
        fragile = (word_p < NOT_FILTERABLE) & (np.abs(cz) <= EPS * np.sqrt(_dot(v, v)))
        fragile |= edge
        # the other floor choice where a coordinate is within EPS of an integer
        nx, ny = live & (np.abs(fx - np.rint(fx)) <= EPS), live & (np.abs(fy - np.rint(fy)) <= EPS)
        x1 = np.where(fx - x0 < 0.5, x0 - 1, x0 + 1)
        y1 = np.where(fy - y0 < 0.5, y0 - 1, y0 + 1)
        for (xa, ya, where) in ((x1, y0, nx), (x0, y1, ny), (x1, y1, nx & ny)):
            if not where.any():
                continue
            alt, _ = _gather(*args, xa, ya, params)
            diff = np.abs(alt - out).max(-1)
            scale = np.maximum(np.abs(alt), np.abs(out)).max(-1)
            fragile |= where & (diff > 1e-3 * scale)
    return out, fragile
