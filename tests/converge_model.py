"""numpy restatement of the error estimate behind sampling to a target error
(include/mrt.h "adaptive sampling"): the mean relative squared
error per tile (mrt_tile_error) and the tiles above a threshold with their
summary (mrt_tile_threshold).

tile_error is evaluated in float32, every operation rounded in the order the
header writes it (the summation order is free: numpy's pairwise sum), or in
float64.  tile_threshold's list and counts are exact; its two floats are
evaluated in `dtype`."""
from __future__ import annotations

import numpy as np

from adaptive_model import TILE, _finite3, tiles_of
from denoise_model import NOT_FILTERABLE, words
from variance_model import lum


def pixel_terms(image, var, guide_n, eps, dtype=np.float32):
    """(term [H, W] of `dtype`, counted [H, W] bool): v / (l l + eps^2) and the pixels that count."""
    T = np.dtype(dtype).type
    image = np.asarray(image, np.float32)
    H, W = image.shape[:2]
    ok = (words(np.asarray(guide_n, np.float32).reshape(H, W, 4)) < NOT_FILTERABLE) & _finite3(image)
    l = lum(image[..., :3], dtype)
    e2 = T(T(np.float32(eps)) * T(np.float32(eps)))
    with np.errstate(all="ignore"):
        term = (np.asarray(var, np.float32).reshape(H, W).astype(T) / ((l * l).astype(T) + e2).astype(T)).astype(T)
    return np.where(ok, term, T(0)), ok


def tile_error(image, var, guide_n, eps, dtype=np.float32):
    """mrt_tile_error: (mean_error [tiles] of `dtype`, pixels [tiles] uint32), row-major over the tiles."""
    T = np.dtype(dtype).type
    term, ok = pixel_terms(image, var, guide_n, eps, dtype)
    H, W = ok.shape
    tx, ty = tiles_of(W, H)
    mean, pixels = np.zeros(tx * ty, T), np.zeros(tx * ty, np.uint32)
    for t in range(tx * ty):
        y, x = t // tx, t % tx
        box = (slice(y * TILE, (y + 1) * TILE), slice(x * TILE, (x + 1) * TILE))
        pixels[t] = int(ok[box].sum())
        if pixels[t]:
            mean[t] = T(term[box].sum(dtype=T) / T(pixels[t]))
    return mean, pixels


def threshold_keys(mean_error, pixels):
    """key(t) in float64 (exact: every float32 is one)."""
    e = np.asarray(mean_error, np.float32).astype(np.float64)
    n = np.asarray(pixels, np.uint32)
    return np.where(np.isfinite(e) & (e > 0) & (n > 0), e, 0.0)


def tile_threshold(mean_error, pixels, threshold, max_count, dtype=np.float32):
    """mrt_tile_threshold: (list, summary dict).  The list holds min(A, max_count) tiles, worst first, ties by
    ascending tile index."""
    T = np.dtype(dtype).type
    key = threshold_keys(mean_error, pixels)
    n = np.asarray(pixels, np.uint32).astype(np.int64)
    above = key > float(np.float32(threshold))
    order = np.lexsort((np.arange(len(key)), -key))
    order = order[above[order]]
    A = int(above.sum())
    total = int(n.sum())
    with np.errstate(all="ignore"):
        weighted = (key.astype(T) * n.astype(T)).astype(T).sum(dtype=T)
        frame = T(weighted / T(total)) if total else T(0)
    summary = {"frame_error": frame, "max_tile_error": np.float32(key.max()), "tiles_above": A,
               "tiles_listed": min(A, int(max_count)), "tiles_counted": int((n > 0).sum()), "pixels": total}
    return order[:max_count].astype(np.uint32), summary
