#!/usr/bin/env python3
"""Time firefly suppression (GPU box) at 1920x1080 on a CornellBox-Water render
with luminance moments and its guide planes: a host clock around 200 enqueued
calls that end in a synchronise, the versions alternating round by round
(median, min and max are printed; the same version's even and odd rounds give
the spread a difference has to exceed).

  one mrt_firefly_clamp per radius 1, 2, 3, beside its compulsory traffic
  (16 B image + 32 B guides read, 16 B written per pixel), the default radius
  again without the counter of changed pixels (no memset, no atomics) and, as a
  yardstick, one LDS-staged iteration of mrt_denoise_variance at step 1;
  mrt_renderer_denoise_variance with the clamp on against off, on one renderer.
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


def alternate(fns, calls, rounds):
    """{name: ms per call of 2 * rounds rounds}, the versions taking turns round by round."""
    series = {k: [] for k in fns}
    for fn in fns.values():
        rounds_ms(fn, 20, 1)
    for _ in range(2 * rounds):
        for k, fn in fns.items():
            series[k] += rounds_ms(fn, calls, 1)
    return series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="CornellBox-Water")
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.calls >= 1 and a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene(a.scene, device=0)
    r = mrt.Renderer(sc, W, H, 4, moments=True)
    r.draw(2)
    r.sync()
    sp = mrt.SvgfParams.default()
    gn, gp, out, counted = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(4))
    var = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    count = torch.zeros(4, dtype=torch.int32, device="cuda")
    mrt.guides(sc, W, H, gn.data_ptr(), gp.data_ptr(), precise=False)
    mrt.temporal_resolve(r.moments_ptr(), 2, None, counted.data_ptr(), W, H)
    mrt.variance(counted.data_ptr(), gn.data_ptr(), gp.data_ptr(), var.data_ptr(), W, H, sp)
    image = r.image_ptr()
    print(f"{a.scene} {W}x{H}, {a.calls} calls per round, {2 * a.rounds} rounds per version", flush=True)

    def clamp_call(R, counted=True):
        p = mrt.FireflyParams.default()
        p.radius = R
        c = count.data_ptr() if counted else None   # without: no 4-byte memset in front of the kernel, no atomic
        return lambda: mrt.firefly_clamp(image, gn.data_ptr(), gp.data_ptr(), out.data_ptr(), c, W, H, p, sync=False)

    fns = {f"clamp R={R}": clamp_call(R) for R in (1, 2, 3)}
    fns["clamp R=2 without the count"] = clamp_call(2, False)
    fns["staged svgf step 1"] = lambda: mrt.debug_denoise_variance_step(
        image, var.data_ptr(), gn.data_ptr(), gp.data_ptr(), out.data_ptr(), W, H, sp, 0, 2, sync=False)
    series = alternate(fns, a.calls, a.rounds)
    traffic = W * H * 64
    for k, v in series.items():
        med = statistics.median(v)
        extra = f" | compulsory traffic {traffic / 1e6:.1f} MB -> {traffic / (med * 1e-3) / 1e12:.3f} TB/s" \
            if k.startswith("clamp") else ""
        print(f"{k}: {fmt(v)} ms | spread (even vs odd rounds) {spread(v) * 100:.2f} %{extra}", flush=True)
    mrt.synchronize()
    print(f"pixels clamped at R=3, 2 frames: {int(count.cpu()[0])} of {W * H}", flush=True)
    base = statistics.median(series["staged svgf step 1"])
    for R in (1, 2, 3):
        print(f"clamp R={R} / staged svgf step 1: {statistics.median(series[f'clamp R={R}']) / base:.3f}", flush=True)

    fp = mrt.FireflyParams.default()

    def whole(on):
        def fn():
            r.set_firefly(fp if on else None)
            r.denoise_variance()
        return fn

    series = alternate({"off": whole(False), "on": whole(True)}, a.calls, a.rounds)
    for k, v in series.items():
        print(f"mrt_renderer_denoise_variance (defaults, 2 frames), clamp {k}: {fmt(v)} ms | spread "
              f"{spread(v) * 100:.2f} %", flush=True)
    print(f"on / off: {statistics.median(series['on']) / statistics.median(series['off']):.4f}, on - off: "
          f"{statistics.median(series['on']) - statistics.median(series['off']):.4f} ms", flush=True)
    r.close()


if __name__ == "__main__":
    main()
