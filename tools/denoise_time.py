#!/usr/bin/env python3
"""Time the denoiser (GPU box): mrt_denoise at 1920x1080 on a cornellbox render
and its guide planes, a host clock around >= 200 enqueued calls that end in a
synchronise, several rounds (median, min and max are printed).

  tools/denoise_time.py            ms per call for 1..5 iterations and for the default parameters at 1, 4
                                   and 64 accumulated frames, the share of the compulsory-traffic bound
                                   (per iteration 16 B colour + 32 B guides read, 16 B written = 64 B per
                                   pixel; 8 TB/s), and one 1-spp draw of the same scene and size
  tools/denoise_time.py --ab       direct against LDS-staged, one iteration at each step 1, 2, 4, 8, 16
                                   alone, the two alternating round by round; the same version's even and
                                   odd rounds give the spread a difference has to exceed
(DESIGN.md "Denoised output")"""
import argparse
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: its bundled HIP runtime is the one libmrt binds to, mrt.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))
import mrt  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BYTES_PER_PIXEL_ITERATION = 64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ab", action="store_true")
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.calls >= 1 and a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene("cornellbox", device=0)
    r = mrt.Renderer(sc, W, H, 4)
    r.draw(1)
    r.sync()
    image = r.image_ptr()
    gn, gp, out, scratch = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(4))
    mrt.guides(sc, W, H, gn.data_ptr(), gp.data_ptr(), precise=False)
    bound_ms = BYTES_PER_PIXEL_ITERATION * W * H / HBM_BYTES_PER_S * 1e3

    def call(params):
        return lambda: mrt.denoise(image, gn.data_ptr(), gp.data_ptr(), out.data_ptr(), scratch.data_ptr(), W, H,
                                   params, sync=False)

    print(f"{W}x{H}, {a.calls} calls per round, {a.rounds} rounds; compulsory traffic {bound_ms * 1e3:.1f} us "
          f"per iteration at 8 TB/s", flush=True)
    if a.ab:
        one = mrt.DenoiseParams.default(1)

        def step_call(k, path):
            return lambda: mrt.debug_denoise_step(image, gn.data_ptr(), gp.data_ptr(), out.data_ptr(),
                                                  scratch.data_ptr(), W, H, one, k, path, sync=False)

        for k in range(5):
            series = {1: [], 2: []}
            staged = (1 << k) <= 4
            for path in (1, 2):   # warm both up at this step
                rounds_ms(step_call(k, path), 20, 1)
            for _ in range(2 * a.rounds):
                for path in (1, 2):
                    series[path] += rounds_ms(step_call(k, path), a.calls, 1)
            d, s = series[1], series[2]
            halves = [abs(statistics.median(v[0::2]) - statistics.median(v[1::2])) / statistics.median(v) for v in (d, s)]
            print(f"step {1 << k:2d}: direct {fmt(d)} ms | {'staged' if staged else 'staged = direct at this step'} "
                  f"{fmt(s)} ms | staged / direct {statistics.median(s) / statistics.median(d):.3f} | "
                  f"spread (same version, even vs odd rounds) direct {halves[0] * 100:.2f} % staged {halves[1] * 100:.2f} %",
                  flush=True)
        return
    rows = [(f"{n} iteration{'s' if n > 1 else ''}", n, None) for n in range(1, 6)]
    rows += [(f"default, {f} frame{'s' if f > 1 else ''}", None, f) for f in (1, 4, 64)]
    frames_drawn = 1
    for label, n, frames in rows:
        if frames is not None and frames > frames_drawn:   # the image the defaults are meant for
            r.draw(frames - frames_drawn)
            r.sync()
            frames_drawn = frames
        p = mrt.DenoiseParams.default(frames if frames is not None else 1)
        if n is not None:
            p.iterations = n
        fn = call(p)
        rounds_ms(fn, 20, 1)
        v = rounds_ms(fn, a.calls, a.rounds)
        m = statistics.median(v)
        print(f"{label:20s} (iterations {p.iterations}, sigma_color {p.sigma_color:.3f}): {fmt(v)} ms per call, "
              f"{m / p.iterations * 1e3:.1f} us per iteration, {100 * bound_ms * p.iterations / m:.1f} % of the "
              f"traffic bound", flush=True)
    r2 = mrt.Renderer(sc, W, H, 4)
    r2.draw(8)
    r2.sync()

    def draw():
        r2.draw_frame()

    def draws(calls, rounds):
        res = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(calls):
                draw()
            r2.sync()
            res.append((time.perf_counter() - t0) * 1e3 / calls)
        return res

    draws(20, 1)
    v = draws(a.calls, a.rounds)
    print(f"one 1-spp draw of cornellbox (L = 4): {fmt(v)} ms", flush=True)
    r2.close()
    r.close()


if __name__ == "__main__":
    main()
