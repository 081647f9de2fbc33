"""numpy restatement of the definitions of adaptive sampling (include/mrt.h
"adaptive sampling"): the merge of two counted images
(mrt_counted_merge), the per-tile priority (mrt_tile_priority), the selection of
the highest-priority tiles (mrt_tile_select), and one refine pass built from
them with variance_model.variance.

The merge and the priority are evaluated in float32, every operation rounded in
the order the header writes it (what the precise build computes; the priority's
summation order is free), or in float64.  The selection is exact."""
from __future__ import annotations

import numpy as np

from denoise_model import NOT_FILTERABLE, words
from variance_model import lum

TILE = 64


def tiles_of(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_mask(W, H, tiles):
    """uint8 [H, W]: 1 on the pixels of the listed tiles (row-major tile indices)."""
    tx, _ = tiles_of(W, H)
    m = np.zeros((H, W), np.uint8)
    for t in np.asarray(tiles, np.int64).reshape(-1):
        y, x = int(t) // tx, int(t) % tx
        m[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE] = 1
    return m


def tile_pixels(W, H, t):
    return int(tile_mask(W, H, [t]).sum())


def _finite3(c):
    return np.isfinite(np.asarray(c)[..., :3]).all(-1)


def counted_merge(a, b, dtype=np.float32):
    """mrt_counted_merge on [..., 4] float32 counted images."""
    T = np.dtype(dtype).type
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    A, B = a32.astype(T), b32.astype(T)
    ha, hb = A[..., 3:4], B[..., 3:4]
    with np.errstate(all="ignore"):
        t = (ha + hb).astype(T)
        rgb = (((ha * A[..., :3]).astype(T) + (hb * B[..., :3]).astype(T)).astype(T) / t).astype(T)
    out = np.concatenate([rgb, t], -1)
    take_a = (b32[..., 3] == 0) | ~_finite3(b32)
    take_b = ~take_a & ((a32[..., 3] == 0) | ~_finite3(a32))
    out[take_b] = B[take_b]
    out[take_a] = A[take_a]
    return out


def tile_priority(image, var, guide_n, eps, dtype=np.float32):
    """mrt_tile_priority: one value per tile, row-major; the terms are summed in `dtype`, pairwise (numpy)."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    tx, ty = tiles_of(W, H)
    ok = (words(np.asarray(guide_n, np.float32).reshape(H, W, 4)) < NOT_FILTERABLE) & _finite3(image)
    l = lum(image[..., :3], dtype)
    e2 = T(T(np.float32(eps)) * T(np.float32(eps)))
    with np.errstate(all="ignore"):
        term = (np.asarray(var, np.float32).reshape(H, W).astype(T) / ((l * l).astype(T) + e2).astype(T)).astype(T)
    term = np.where(ok, term, T(0))
    out = np.zeros(tx * ty, T)
    for t in range(tx * ty):
        y, x = t // tx, t % tx
        out[t] = term[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE].sum(dtype=T)
    return out


def tile_select(priority, count):
    """mrt_tile_select: the `count` tiles of highest priority, ties by ascending tile index."""
    p = np.asarray(priority, np.float32).astype(np.float64)
    key = np.where(np.isfinite(p) & (p > 0), p, 0.0)
    order = np.lexsort((np.arange(len(key)), -key))
    return order[:count].astype(np.uint32)


def accumulate64(stored, c, n):
    """accumulate_value in float64: c + (stored - c) n / (n + 1); n == 0 overwrites (n per pixel)."""
    n = np.asarray(n, np.float64)[..., None]
    return np.where(n > 0, c + (stored - c) * (n / (n + 1.0)), c)
