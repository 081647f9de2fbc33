#!/usr/bin/env python3
"""Time variance-guided denoising (GPU box) at 1920x1080 on a cornellbox render
with luminance moments and its guide planes: a host clock around >= 200
enqueued calls that end in a synchronise, several rounds (median, min and max
are printed).

  tools/variance_time.py           mrt_variance (counts below and from min_frames on: the spatial and the
                                   temporal estimate), then one iteration of mrt_denoise_variance at each
                                   step 1, 2, 4, 8, 16, direct against LDS-staged, the two alternating round
                                   by round; the same version's even and odd rounds give the spread a
                                   difference has to exceed; then the whole mrt_renderer_denoise_variance
  tools/variance_time.py --draw    the draw rate with and without MRT_FLAG_MOMENTS: two renderers at
                                   --w x --h, L = 4, --spp frames per draw, alternating draw by draw
"""
import argparse
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: its bundled HIP runtime is the one libmrt binds to, mrt.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))
import mrt  # noqa: E402


def rounds_ms(fn, calls, rounds):
    """ms per call of each round: `calls` enqueues, then one synchronise."""
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        mrt.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def fmt(v):
    return f"median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f}"


def spread(v):
    return abs(statistics.median(v[0::2]) - statistics.median(v[1::2])) / statistics.median(v)


def draw_rate(sc, W, H, spp, rounds):
    rs = {flag: mrt.Renderer(sc, W, H, 4, moments=flag) for flag in (False, True)}
    rate = {False: [], True: []}
    for r in rs.values():   # warm up: noise tables, first launches
        r.draw(spp)
        r.sync()
    for _ in range(2 * rounds):
        for flag, r in rs.items():
            t0 = time.perf_counter()
            r.draw(spp)
            r.sync()
            rate[flag].append(W * H * spp / (time.perf_counter() - t0) / 1e6)
    for flag in (False, True):
        v = rate[flag]
        print(f"{W}x{H} {spp} spp L=4 {'with   ' if flag else 'without'} MRT_FLAG_MOMENTS: {fmt(v)} Mpaths/s, "
              f"spread (even vs odd rounds) {spread(v) * 100:.2f} %", flush=True)
    print(f"with / without: {statistics.median(rate[True]) / statistics.median(rate[False]):.4f}", flush=True)
    for r in rs.values():
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--draw", action="store_true")
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.calls >= 1 and a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene("cornellbox", device=0)
    if a.draw:
        draw_rate(sc, W, H, a.spp, a.rounds)
        return
    r = mrt.Renderer(sc, W, H, 4, moments=True)
    r.draw(2)
    r.sync()
    p = mrt.SvgfParams.default()
    gn, gp, out, counted = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    mrt.guides(sc, W, H, gn.data_ptr(), gp.data_ptr(), precise=False)
    print(f"{W}x{H}, {a.calls} calls per round, {a.rounds} rounds", flush=True)
    for frames, what in ((2, "spatial estimate (n < min_frames)"), (16, "temporal estimate (n >= min_frames)")):
        mrt.temporal_resolve(r.moments_ptr(), frames, None, counted.data_ptr(), W, H)   # the same moments, counted so

        def fn():
            mrt.variance(counted.data_ptr(), gn.data_ptr(), gp.data_ptr(), var.data_ptr(), W, H, p, sync=False)

        rounds_ms(fn, 20, 1)
        print(f"mrt_variance, {what}: {fmt(rounds_ms(fn, a.calls, a.rounds))} ms", flush=True)
    mrt.temporal_resolve(r.moments_ptr(), 2, None, counted.data_ptr(), W, H)
    mrt.variance(counted.data_ptr(), gn.data_ptr(), gp.data_ptr(), var.data_ptr(), W, H, p)
    image = r.image_ptr()

    def step_call(k, path):
        return lambda: mrt.debug_denoise_variance_step(image, var.data_ptr(), gn.data_ptr(), gp.data_ptr(),
                                                       out.data_ptr(), W, H, p, k, path, sync=False)

    for k in range(5):
        series = {1: [], 2: []}
        staged = (1 << k) <= 4
        for path in (1, 2):   # warm both up at this step
            rounds_ms(step_call(k, path), 20, 1)
        for _ in range(2 * a.rounds):
            for path in (1, 2):
                series[path] += rounds_ms(step_call(k, path), a.calls, 1)
        d, s = series[1], series[2]
        print(f"step {1 << k:2d}: direct {fmt(d)} ms | {'staged' if staged else 'staged = direct at this step'} "
              f"{fmt(s)} ms | staged / direct {statistics.median(s) / statistics.median(d):.3f} | "
              f"spread (same version, even vs odd rounds) direct {spread(d) * 100:.2f} % staged {spread(s) * 100:.2f} %",
              flush=True)

    def whole():
        r.denoise_variance()

    rounds_ms(whole, 20, 1)
    print(f"mrt_renderer_denoise_variance (defaults, 2 frames): {fmt(rounds_ms(whole, a.calls, a.rounds))} ms",
          flush=True)
    r.close()


if __name__ == "__main__":
    main()
