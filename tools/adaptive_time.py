#!/usr/bin/env python3
"""Time adaptive sampling (GPU box) at 1920x1080, L = 4: a host clock around
enqueued calls that end in a synchronise, the variants alternating round by
round in one call; medians, and the same variant's even against odd rounds as
the spread a difference has to exceed.

  tools/adaptive_time.py            cornellbox (stream kernel): the cost of a tile-frame in draw_tiles with
                                    K = T, T/4 and T/16 tiles against a full draw of the same frames (K = T is
                                    the price of the list instantiation alone); mrt_variance + mrt_tile_priority
                                    + mrt_tile_select; a whole refine(--frames, T/4)
  tools/adaptive_time.py --water    CornellBox-Water (path kernel): the full draw against draw_tiles with K = T/4
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: its bundled HIP runtime is the one libmrt binds to, mrt.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))
import mrt  # noqa: E402


def fmt(v):
    return f"median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f}"


def spread(v):
    return abs(statistics.median(v[0::2]) - statistics.median(v[1::2])) / statistics.median(v)


def timed(r, fn):
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def spaced_tiles(T, K, rng):
    """K distinct tiles spread over the frame (a refine's list is scattered, not a corner)."""
    return np.sort(rng.choice(T, K, replace=False)).astype(np.uint32)


def tile_frame_cost(r, W, H, frames, rounds, counts):
    """us per tile-frame of draw(frames) and of draw_tiles(K tiles, frames), alternating round by round."""
    T = r.tile_count()
    rng = np.random.default_rng(1)
    variants = {"draw": (T, lambda: r.draw(frames))}
    for K in counts:
        lst = np.arange(T, dtype=np.uint32) if K == T else spaced_tiles(T, K, rng)
        variants[f"draw_tiles K={K}"] = (K, (lambda l: lambda: r.draw_tiles(l, frames))(lst))
    series = {k: [] for k in variants}
    for _, fn in variants.values():   # warm up: noise chunks of both schedules, first launches, E / EM
        timed(r, fn)
    for _ in range(2 * rounds):
        for name, (K, fn) in variants.items():
            series[name].append(timed(r, fn) * 1e3 / (K * frames))
    base = statistics.median(series["draw"])
    for name, v in series.items():
        K = variants[name][0]
        print(f"{W}x{H} L=4 {frames} frames, {name:22s} ({K:4d} of {T} tiles): {fmt(v)} us per tile-frame, "
              f"x{statistics.median(v) / base:.4f} of draw, call {statistics.median(v) * K * frames / 1e3:.3f} ms, "
              f"spread (even vs odd rounds) {spread(v) * 100:.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--water", action="store_true")
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene("CornellBox-Water" if a.water else "cornellbox", device=0)
    r = mrt.Renderer(sc, W, H, 4, moments=True)
    T = r.tile_count()
    print(f"{'CornellBox-Water' if a.water else 'cornellbox'} kernel {r.stats()['kernel']}, {T} tiles", flush=True)
    if a.water:
        tile_frame_cost(r, W, H, a.frames, a.rounds, [max(1, T // 4)])
        r.close()
        return
    tile_frame_cost(r, W, H, a.frames, a.rounds, [T, max(1, T // 4), max(1, T // 16)])
    # the choice: variance, priority, selection on the stage level, enqueued back to back
    r.reset()
    r.draw(4)
    r.denoise_variance()
    r.sync()
    p, q = mrt.SvgfParams.default(), mrt.AdaptiveParams.default()
    gn, gp, res, mres = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    pri = torch.zeros(T, dtype=torch.float32, device="cuda")
    lst = torch.zeros(T, dtype=torch.int32, device="cuda")
    mrt.guides(sc, W, H, gn.data_ptr(), gp.data_ptr(), precise=False)
    mrt.temporal_resolve(r.image_ptr(), 4, None, res.data_ptr(), W, H)
    mrt.temporal_resolve(r.moments_ptr(), 4, None, mres.data_ptr(), W, H)
    steps = {
        "mrt_variance": lambda: mrt.variance(mres.data_ptr(), gn.data_ptr(), gp.data_ptr(), var.data_ptr(), W, H, p, sync=False),
        "mrt_tile_priority": lambda: mrt.tile_priority(res.data_ptr(), var.data_ptr(), gn.data_ptr(), pri.data_ptr(), W, H, q,
                                                       precise=False, sync=False),
        "mrt_tile_select": lambda: mrt.tile_select(pri.data_ptr(), T, max(1, T // 4), lst.data_ptr(), sync=False),
    }
    steps["priority + select"] = lambda: (steps["mrt_tile_priority"](), steps["mrt_tile_select"]())
    for name, fn in steps.items():
        v = []
        for _ in range(a.rounds + 1):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            mrt.synchronize()
            v.append((time.perf_counter() - t0) * 1e3 / a.calls)
        print(f"{name}: {fmt(v[1:])} ms per call ({a.calls} calls per round)", flush=True)
    # a whole pass: refine(frames, T/4) against draw_tiles of as many tiles (the choice's share)
    K = max(1, T // 4)
    fixed = spaced_tiles(T, K, np.random.default_rng(2))
    series = {"refine": [], "draw_tiles": []}
    timed(r, lambda: r.refine(a.frames, K))
    for _ in range(2 * a.rounds):
        series["refine"].append(timed(r, lambda: r.refine(a.frames, K)))
        series["draw_tiles"].append(timed(r, lambda: r.draw_tiles(fixed, a.frames)))
    for name, v in series.items():
        print(f"{name}({a.frames} frames, {K} tiles): {fmt(v)} ms, spread (even vs odd rounds) {spread(v) * 100:.2f} %", flush=True)
    print(f"refine / draw_tiles: {statistics.median(series['refine']) / statistics.median(series['draw_tiles']):.4f}; "
          f"refine_stats {r.refine_stats()}", flush=True)
    r.close()


if __name__ == "__main__":
    main()
