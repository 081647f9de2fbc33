#!/usr/bin/env python3
"""Time the temporal history kernels (GPU box): mrt_reproject and
mrt_temporal_resolve at 1920x1080 on a cornellbox render and its guide planes
for the cameras A -> D of tests/camera_cases.py, a host clock around >= 200
enqueued calls that end in a synchronise, several rounds (median, min and max
are printed; the calls run back to back, so their buffers, 199 MB for a
reproject, stay in the 256 MiB Infinity Cache: warm-cache figures), against
the compulsory traffic at 8 TB/s —
  reproject: 16 B previous colour + 32 B previous guides + 32 B current guides
             read, 16 B written = 96 B per pixel
  resolve:   16 B image + 16 B history read, 16 B written = 48 B per pixel
— beside one 1-spp draw of the same scene and size, one guide pass, and a
whole mrt_renderer_set_camera and mrt_renderer_move_camera (host side included)
(DESIGN.md "Temporal reprojection")."""
import argparse
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: its bundled HIP runtime is the one libmrt binds to, mrt.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mrt  # noqa: E402
from camera_cases import camera  # noqa: E402  (the tests' cameras A and D)

HBM_BYTES_PER_S = 8.0e12


def rounds_ms(fn, calls, rounds, sync=mrt.synchronize):
    """ms per call of each round: `calls` enqueues, then one synchronise."""
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
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
    a = ap.parse_args()
    W, H = a.w, a.h
    assert a.calls >= 1 and a.rounds >= 2
    torch.zeros(1, device="cuda")
    sc = mrt.Scene("cornellbox", device=0)
    A, D = camera(mrt, "A"), camera(mrt, "D")
    r = mrt.Renderer(sc, W, H, 4)
    r.set_camera(A)
    r.draw(4)
    r.sync()
    image = r.image_ptr()
    an, ap_, dn, dp, prev, hist, out = (torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(7))
    mrt.guides(sc, W, H, an.data_ptr(), ap_.data_ptr(), camera=A, precise=False)
    mrt.guides(sc, W, H, dn.data_ptr(), dp.data_ptr(), camera=D, precise=False)
    params = mrt.ReprojectParams.default()
    mrt.temporal_resolve(image, 4, None, prev.data_ptr(), W, H)

    def reproject():
        mrt.reproject(prev.data_ptr(), an.data_ptr(), ap_.data_ptr(), A, dn.data_ptr(), dp.data_ptr(), hist.data_ptr(),
                      W, H, params, sync=False)

    def resolve():
        mrt.temporal_resolve(image, 4, hist.data_ptr(), out.data_ptr(), W, H, sync=False)

    reproject()
    mrt.synchronize()
    carried = float((hist.view(-1, 4)[:, 3] > 0).float().mean())
    print(f"{W}x{H}, {a.calls} calls per round, {a.rounds} rounds; cameras A -> D, history on {carried:.3f} of the pixels",
          flush=True)
    for label, fn, bytes_per_pixel in (("reproject", reproject, 96), ("resolve", resolve, 48)):
        bound_ms = bytes_per_pixel * W * H / HBM_BYTES_PER_S * 1e3
        rounds_ms(fn, 20, 1)
        v = rounds_ms(fn, a.calls, a.rounds)
        m = statistics.median(v)
        print(f"{label:10s}: {fmt(v)} ms per call; compulsory traffic {bytes_per_pixel} B per pixel = "
              f"{bound_ms * 1e3:.1f} us at 8 TB/s: {100 * bound_ms / m:.1f} % of the traffic bound (warm cache)", flush=True)
    r2 = mrt.Renderer(sc, W, H, 4)
    r2.set_camera(A)
    r2.draw(8)
    r2.sync()
    rounds_ms(r2.draw_frame, 20, 1, r2.sync)
    v = rounds_ms(r2.draw_frame, a.calls, a.rounds, r2.sync)
    print(f"one 1-spp draw of cornellbox (L = 4, camera A): {fmt(v)} ms", flush=True)
    cams = [D, A]

    def move():
        r2.move_camera(cams[0])
        cams.reverse()

    def set_camera():
        r2.set_camera(cams[0])
        cams.reverse()

    def guide_pass():
        mrt.guides(sc, W, H, dn.data_ptr(), dp.data_ptr(), camera=D, precise=False, sync=False)

    # a move in a row of moves traces one guide pass (the planes of the camera it leaves are current)
    for label, fn, sync in (("mrt_guides (camera D)", guide_pass, mrt.synchronize),
                            ("mrt_renderer_set_camera (host: candidate lists + upload)", set_camera, r2.sync),
                            ("mrt_renderer_move_camera (set_camera + guide pass + resolve + reproject)", move, r2.sync)):
        r2.draw(1)   # something to carry: the first move makes the history the later ones carry on
        rounds_ms(fn, 4, 1, sync)
        v = rounds_ms(fn, max(2, a.calls // 10), a.rounds, sync)
        print(f"one {label}: {fmt(v)} ms", flush=True)
    r2.close()
    r.close()


if __name__ == "__main__":
    main()
