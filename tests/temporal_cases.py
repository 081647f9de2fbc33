"""Synthetic inputs shared by the temporal-history tests: guide planes ray-cast
analytically (numpy, float64, stored as float32) from a pinhole camera over a
floor, a back wall and a floating quad in front of the wall that disoccludes
when the camera moves — each with its own material word — plus a strip of
misses and a block of light-flagged pixels, and a seeded counted image."""
from __future__ import annotations

import numpy as np

from denoise_model import MISS_WORD, NOT_FILTERABLE

UP = (0.0, 1.0, 0.0)
# name: (eye, target, fov_x_degrees)
EYES = {
    "A": ((0.1, 1.0, 2.6), (0.0, 0.8, 0.0), 60.0),
    "shift": ((0.22, 1.06, 2.5), (0.12, 0.86, -0.1), 60.0),      # A translated (same orientation)
    "turn": ((0.1, 1.0, 2.6), (0.25, 0.7, 0.0), 50.0),           # A rotated, narrower view
    "pan": ((0.1, 1.0, 2.6), (1.5, 0.8, 0.0), 60.0),             # A rotated by about 30 degrees: taps leave the image
    "behind": ((0.0, 1.0, -4.0), (0.0, 1.0, -8.0), 60.0),        # beyond the wall, looking away: sees nothing
}
# (name, previous camera, current camera)
PAIRS = [("identical", "A", "A"), ("translated", "A", "shift"), ("rotated", "A", "turn"),
         ("behind", "behind", "A"), ("pan", "A", "pan")]
SIZES = [(53, 37), (64, 64), (5, 3), (2, 2)]

# (axis, offset, normal, word, bounds of the two other axes)
SURFACES = [
    (1, 0.0, (0.0, 1.0, 0.0), 0, ((-2.0, 2.0), (-1.5, 3.0))),      # floor y = 0: x, z
    (2, -1.5, (0.0, 0.0, 1.0), 1, ((-2.0, 2.0), (0.0, 2.2))),      # wall z = -1.5: x, y
    (2, 0.3, (0.0, 0.0, 1.0), 2, ((-0.4, 0.5), (0.5, 1.2))),       # quad z = 0.3: x, y
]


def camera(mrt_mod, name):
    eye, target, fov = EYES[name]
    return mrt_mod.Camera.look_at(eye, target, UP, fov)


def raycast(cam, W, H):
    """(guide_n, guide_p) float32 [H, W, 4], in mrt_guides' record layout, of
    the pixel-centre rays of `cam`."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = float(cam.tan_half_fov)
    o = np.array(list(cam.origin), np.float64)
    right, up, fwd = (np.array(list(a), np.float64) for a in (cam.right, cam.up, cam.forward))
    cx = (2.0 * x / (W - 1) - 1.0) * s
    cy = (2.0 * y / (H - 1) - 1.0) * (H / W) * s
    d = right * cx[..., None] + up * cy[..., None] + fwd
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((H, W), np.inf)
    word = np.full((H, W), MISS_WORD, np.uint32)
    nrm = np.zeros((H, W, 3))
    for axis, off, normal, w, bounds in SURFACES:
        with np.errstate(all="ignore"):
            t = (off - o[axis]) / d[..., axis]
            pos = o + t[..., None] * d
        others = [k for k in range(3) if k != axis]
        hit = np.isfinite(t) & (t > 1e-6) & (t < best)
        for k, (lo, hi) in zip(others, bounds):
            hit &= (pos[..., k] >= lo) & (pos[..., k] <= hi)
        best = np.where(hit, t, best)
        word = np.where(hit, np.uint32(w), word)
        nrm = np.where(hit[..., None], np.array(normal), nrm)
    hit = np.isfinite(best)
    if H >= 8:                 # a strip of misses
        hit[H - 2:] = False
        word[H - 2:] = MISS_WORD
    if H >= 8 and W >= 16:     # a block of light-flagged pixels
        word[H // 2 - 2:H // 2 + 2, W // 4 - 3:W // 4 + 3] |= np.uint32(NOT_FILTERABLE)
    tt = np.where(hit, best, 0.0)
    gn = np.zeros((H, W, 4), np.float32)
    gp = np.zeros((H, W, 4), np.float32)
    gn[..., :3] = np.where(hit[..., None], nrm, 0.0)
    gn[..., 3] = word.view(np.float32)
    gp[..., :3] = np.where(hit[..., None], o + tt[..., None] * d, 0.0)
    gp[..., 3] = np.where(hit, best, -1.0)
    return gn, gp


def counted_image(W, H, seed):
    """A counted image: rgb in [0, 2], counts in (0, 40]; about 1 % of the
    pixels (one at least, from 15 pixels on) with count 0 and rgb 0, and, where
    the size has room, one NaN and one Inf pixel."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, size=(H, W, 4)).astype(np.float32)
    img[..., 3] = rng.uniform(0.01, 40.0, size=(H, W)).astype(np.float32)
    if W * H >= 15:
        k = max(1, round(0.01 * W * H))
        idx = rng.choice(W * H, size=k, replace=False)
        img.reshape(-1, 4)[idx] = 0.0
    if W >= 16 and H >= 8:
        img[H // 3, W // 2, 1] = np.nan
        img[H // 3 + 1, W // 3, 0] = np.inf
    return img


def case(mrt_mod, pair, W, H):
    """(prev, prev_n, prev_p, prev_cam, cur_n, cur_p) of a camera pair."""
    _, a, b = next(p for p in PAIRS if p[0] == pair)
    ca, cb = camera(mrt_mod, a), camera(mrt_mod, b)
    pn, pp = raycast(ca, W, H)
    cn, cp = raycast(cb, W, H)
    return counted_image(W, H, 100 * W + H), pn, pp, ca, cn, cp


def fragile_limit(W, H):
    """At most 2 % of the pixels, or 1 pixel, whichever is larger."""
    return max(1, int(0.02 * W * H))
