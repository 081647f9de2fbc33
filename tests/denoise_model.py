"""numpy restatement of the denoiser's two definitions (include/mrt.h "denoised
output", DESIGN.md "Denoised output"): the record layout of the first-hit guide
planes, and the edge-avoiding A-Trous filter.

guides_from_hits evaluates the planes in float32 with the kernels' operation
order (shade_hit's interpolation), so the precise build can be compared bit for
bit.  atrous evaluates the filter in float32 or float64, taps in the order
dy = -2..2 (outer), dx = -2..2 (inner)."""
from __future__ import annotations

import numpy as np

KERNEL = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
NOT_FILTERABLE = 0x80000000
MISS_WORD = 0xFFFFFFFF


def _field(scene, name):
    return scene[name] if isinstance(scene, dict) else getattr(scene, name)


def guides_from_hits(export, isect, rays=None):
    """(guide_n, guide_p), float32 [N, 4] each, from nearest hits (oracle
    ISECT_DTYPE records of the guide rays `rays`, which only fix N) and the
    scene's reference-layout arrays (mrt.Scene.export() or an OracleScene):
    guide_n = (normal, bits(word)), guide_p = (position, t)."""
    isect = np.ascontiguousarray(isect)
    n = len(isect)
    assert rays is None or len(rays) == n
    V, R = _field(export, "vertices"), _field(export, "references")
    f32 = np.float32
    hit = isect["distance"] >= 0
    prim = np.where(hit, isect["triangleIndex"], 0).astype(np.int64)
    u, v = isect["coordinates"][:, 0].astype(f32), isect["coordinates"][:, 1].astype(f32)
    w = (f32(1.0) - u) - v
    tri = R["tri"][prim].astype(np.int64)                     # [n, 3] vertex indices
    P = [V["v"][tri[:, k]].astype(f32) for k in range(3)]
    N = [V["n"][tri[:, k]].astype(f32) for k in range(3)]
    with np.errstate(all="ignore"):
        x = (P[0] * u[:, None] + P[1] * v[:, None]) + P[2] * w[:, None]
        m = (N[0] * u[:, None] + N[1] * v[:, None]) + N[2] * w[:, None]
        d = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        nn = m * (f32(1.0) / np.sqrt(d))[:, None]
    word = R["materialIndex"][prim].astype(np.uint32)
    word = np.where(R["lightTriangleIndex"][prim] != MISS_WORD, word | np.uint32(NOT_FILTERABLE), word)
    gn = np.zeros((n, 4), f32)
    gp = np.zeros((n, 4), f32)
    gn[:, :3] = np.where(hit[:, None], nn, f32(0.0))
    gn[:, 3] = np.where(hit, word, np.uint32(MISS_WORD)).astype(np.uint32).view(f32)
    gp[:, :3] = np.where(hit[:, None], x, f32(0.0))
    gp[:, 3] = np.where(hit, isect["distance"].astype(f32), f32(-1.0))
    return gn, gp


def words(guide_n):
    return np.ascontiguousarray(guide_n[..., 3]).view(np.uint32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def atrous(image, guide_n, guide_p, params, dtype=np.float64):
    """The filter on image [H, W, 4] float32 with guide planes [H, W, 4]
    float32; params has iterations, sigma_color, sigma_plane,
    normal_log2_power.  Returns [H, W, 4] of `dtype` (alpha copied)."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    word = words(np.asarray(guide_n, np.float32).reshape(H, W, 4))
    filt = word < NOT_FILTERABLE
    n = np.asarray(guide_n, np.float32).reshape(H, W, 4)[..., :3].astype(T)
    x = np.asarray(guide_p, np.float32).reshape(H, W, 4)[..., :3].astype(T)
    t = np.asarray(guide_p, np.float32).reshape(H, W, 4)[..., 3].astype(T)
    c = image[..., :3].astype(T)
    sigma_c, sigma_p = T(np.float32(params.sigma_color)), T(np.float32(params.sigma_plane))
    e = int(params.normal_log2_power)
    with np.errstate(all="ignore"):
        for i in range(int(params.iterations)):
            s = 1 << i
            fin = np.isfinite(c).all(-1)
            sw = np.zeros((H, W), T)
            sc = np.zeros((H, W, 3), T)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1 = max(0, -dy * s), min(H, H - dy * s)
                    x0, x1 = max(0, -dx * s), min(W, W - dx * s)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    Pp = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    ok = filt[Pp] & (word[Q] == word[Pp]) & fin[Q]
                    D = np.fmax(T(0.0), _dot(n[Pp], n[Q]))   # fmaxf: 0 for a NaN product
                    for _ in range(e):
                        D = D * D
                    dist = np.abs(_dot(n[Pp], x[Q] - x[Pp]))
                    wgt = (T(KERNEL[dx + 2]) * T(KERNEL[dy + 2])) * D * np.exp(-dist / (sigma_p * t[Pp]))
                    if sigma_c > 0:
                        dc = c[Q] - c[Pp]
                        wgt = wgt * np.where(fin[Pp], np.exp(-_dot(dc, dc) / (sigma_c * sigma_c)), T(1.0))
                    wgt = np.where(ok, wgt, T(0.0)).astype(T)
                    cq = np.where(ok[..., None], c[Q], T(0.0))
                    sw[Pp] += wgt
                    sc[Pp] += wgt[..., None] * cq
            use = filt & (sw > 0)
            c = np.where(use[..., None], sc / np.where(use, sw, T(1.0))[..., None], c).astype(T)
    out = image.astype(T)
    out[..., :3] = c
    return out


def rel_mse(a, b):
    """mean((a - b)^2 / (b^2 + 1e-2)) over RGB."""
    a, b = np.asarray(a, np.float64)[..., :3], np.asarray(b, np.float64)[..., :3]
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))
