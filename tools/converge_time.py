#!/usr/bin/env python3
"""Time sampling to a target error (GPU box) at 1920x1080, L = 4 on cornellbox:
a host clock around calls that end in a synchronise, the variants alternating
round by round in one call; medians, and the same variant's even against odd
rounds as the spread a difference has to exceed.

  one estimate (mrt_renderer_error: denoise_variance + mrt_tile_error + mrt_tile_threshold + the summary's
  round trip) against denoise_variance alone, which it contains; the two new stage calls alone, enqueued
  back to back; a whole converge against draw_tiles of the same tiles and frames, pass by pass
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--base", type=int, default=8, help="frames drawn before the estimates")
    ap.add_argument("--frames", type=int, default=8, help="frames per converge pass")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene("cornellbox", device=0)
    r = mrt.Renderer(sc, W, H, 4, moments=True)
    T = r.tile_count()
    print(f"cornellbox kernel {r.stats()['kernel']}, {W}x{H}, {T} tiles, {a.base} base frames", flush=True)
    r.draw(a.base)
    r.sync()
    # one estimate against the denoise it contains
    variants = {"error_estimate": lambda: r.error_estimate(0.0), "denoise_variance": r.denoise_variance}
    series = {k: [] for k in variants}
    for fn in variants.values():
        timed(r, fn)
    for _ in range(2 * a.rounds):
        for name, fn in variants.items():
            series[name].append(timed(r, fn))
    for name, v in series.items():
        print(f"{name}: {fmt(v)} ms, spread (even vs odd rounds) {spread(v) * 100:.2f} %", flush=True)
    d = statistics.median(series["error_estimate"]) - statistics.median(series["denoise_variance"])
    print(f"error_estimate - denoise_variance: {d:.4f} ms (tile_error + tile_threshold + the summary's round trip)", flush=True)
    s = r.error_estimate(0.0)
    print(f"summary {s}", flush=True)
    # the two stage calls alone
    gn, gp, den = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(3))
    var = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    mrt.guides(sc, W, H, gn.data_ptr(), gp.data_ptr(), precise=False)
    den.copy_(torch.from_numpy(r.read_denoised().reshape(-1)))
    var.copy_(torch.from_numpy(r.read_variance().reshape(-1)))
    err = torch.zeros(T, dtype=torch.float32, device="cuda")
    pix, lst = (torch.zeros(T, dtype=torch.int32, device="cuda") for _ in range(2))
    summ = torch.zeros(8, dtype=torch.int32, device="cuda")
    q = mrt.AdaptiveParams.default()
    thr = 0.5 * s["max_tile_error"]
    steps = {
        "mrt_tile_error": lambda: mrt.tile_error(den.data_ptr(), var.data_ptr(), gn.data_ptr(), err.data_ptr(), pix.data_ptr(),
                                                 W, H, q, precise=False, sync=False),
        "mrt_tile_threshold": lambda: mrt.tile_threshold(err.data_ptr(), pix.data_ptr(), T, thr, T, lst.data_ptr(),
                                                         summ.data_ptr(), sync=False),
    }
    steps["error + threshold"] = lambda: (steps["mrt_tile_error"](), steps["mrt_tile_threshold"]())
    for name, fn in steps.items():
        v = []
        for _ in range(a.rounds + 1):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            mrt.synchronize()
            v.append((time.perf_counter() - t0) * 1e3 / a.calls)
        print(f"{name}: {fmt(v[1:])} ms per call ({a.calls} calls per round)", flush=True)
    # a whole converge against the same tile-frames drawn by draw_tiles: each round on a fresh accumulation,
    # the replay drawing pass by pass the lists the converge of that round chose
    target = 0.5 * s["max_tile_error"]
    series = {"converge": [], "draw_tiles": []}
    info = None
    for k in range(2 * a.rounds + 1):
        r.reset()
        r.draw(a.base)
        r.sync()
        lists = []
        t0 = time.perf_counter()
        res = r.converge(target_error=target, frames_per_pass=a.frames, max_passes=8)
        r.sync()
        tc = (time.perf_counter() - t0) * 1e3
        # the lists cannot be read between the passes of one call: take them from a stepwise run of the same loop
        r.reset()
        r.draw(a.base)
        for _ in range(res["passes"]):
            r.error_estimate(target)
            lists.append(r.read_tile_list())
            r.draw_tiles(lists[-1], a.frames)
        r.reset()
        r.draw(a.base)
        r.sync()
        t0 = time.perf_counter()
        for l in lists:
            r.draw_tiles(l, a.frames)
        r.sync()
        td = (time.perf_counter() - t0) * 1e3
        if k:   # (round 0 warms up)
            series["converge"].append(tc)
            series["draw_tiles"].append(td)
        info = (res, [len(l) for l in lists])
    res, sizes = info
    print(f"converge(target {target:.5g}, {a.frames} frames per pass): {res['passes']} passes of {sizes} tiles, "
          f"{res['tile_frames']} tile-frames, converged {res['converged']}, frame error "
          f"{res['first']['frame_error']:.5g} -> {res['last']['frame_error']:.5g}", flush=True)
    for name, v in series.items():
        print(f"{name}: {fmt(v)} ms, spread (even vs odd rounds) {spread(v) * 100:.2f} %", flush=True)
    c, d = statistics.median(series["converge"]), statistics.median(series["draw_tiles"])
    print(f"converge / draw_tiles: {c / d:.4f}; the estimates' share {c - d:.3f} ms over {res['passes'] + 1} estimates",
          flush=True)
    r.close()


if __name__ == "__main__":
    main()
