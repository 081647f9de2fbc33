#!/usr/bin/env python3
"""Time moving geometry (GPU box).  Device times are taken with HIP events
(hipEventRecord on the stream the work runs on, hipEventElapsedTime), host times
with a host clock; the two sides of each comparison alternate round by round and
every round is printed, so the spread a difference has to exceed is on the line.

  mrt_guides_motion against mrt_guides        device ms per call: events around `--calls` enqueued calls;
                                              beside it the host clock around the same calls and a sync
  mrt_renderer_move_scene against             device ms from an event recorded before the call to one recorded
    mrt_renderer_move_camera                  behind it on the renderer's stream (move_scene's includes the
                                              stream's idle time across its one host wait), and the host ms
                                              of the call and a sync; one frame drawn between moves; the scene
                                              moves A -> B -> A ..., the camera between two poses
  mrt_renderer_set_scene                      host ms of the call alone

at 1920x1080 on cornellbox against a copy with the short box translated, and on
cornellbox + 1 << 20 procedural triangles, seed 1 against seed 2 (device PLOC
builder: the deep tree, so the guide passes run their spill variant).
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

import torch  # noqa: F401  (first: its bundled HIP runtime is the one libmrt binds to, mrt.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "metal-renderer_amd"))
import mrt  # noqa: E402

SHIFT = (0.15, 0.0, 0.1)


def hip_runtime():
    """The HIP runtime this process has loaded (the one libmrt's calls go to)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


class Timer:
    """Two HIP events on `stream` (None: the null stream, where the stage calls run)."""

    def __init__(self, hip, stream=None):
        self.hip, self.stream = hip, ctypes.c_void_p(stream)
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert hip.hipEventCreate(ctypes.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0

    def stop_ms(self):
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def moved_cornellbox(directory):
    """cornellbox.obj with the eight vertices of the shortBox faces translated by SHIFT"""
    with open(mrt.scene_path("cornellbox")) as f:
        lines = f.read().splitlines()
    used, inside = set(), False
    for line in lines:
        if line.startswith("usemtl "):
            inside = line.split()[1] == "shortBox"
        elif line.startswith("f ") and inside:
            used |= {int(c.split("/")[0]) for c in line.split()[1:]}
    k = 0
    for i, line in enumerate(lines):
        if line.startswith("v "):
            k += 1
            if k in used:
                x, y, z = (float(t) for t in line.split()[1:4])
                lines[i] = f"v  {x + SHIFT[0]:.5f} {y + SHIFT[1]:.5f} {z + SHIFT[2]:.5f}"
    path = os.path.join(directory, "cornellbox_moved.obj")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def fmt(v):
    return f"median {statistics.median(v):.4f} [" + " ".join(f"{x:.4f}" for x in v) + "]"


def alternate(fns, rounds):
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(fn())
    return out


def measure(a, hip, name, A, B):
    W, H = a.w, a.h
    planes = [torch.zeros(W * H * 4, dtype=torch.float32, device="cuda") for _ in range(4)]
    p = [t.data_ptr() for t in planes]
    null = Timer(hip)
    print(f"{name}: traversal stack entries {A.info['bvh_max_stack']} / {B.info['bvh_max_stack']}", flush=True)

    def stage(fn):
        def run():
            t0 = time.perf_counter()
            null.start()
            for _ in range(a.calls):
                fn()
            dev = null.stop_ms() / a.calls
            return dev, (time.perf_counter() - t0) * 1e3 / a.calls
        return run

    calls = {"mrt_guides": stage(lambda: mrt.guides(B, W, H, p[0], p[1], precise=False, sync=False)),
             "mrt_guides_motion": stage(lambda: mrt.guides_motion(B, A, W, H, *p, precise=False, sync=False))}
    for fn in calls.values():   # warm both
        fn()
    for k, v in alternate(calls, a.rounds).items():
        print(f"{name}: {k} device ms {fmt([d for d, _ in v])}; host ms {fmt([h for _, h in v])} "
              f"({a.calls} calls per round)", flush=True)

    C = [mrt.Camera.default(), mrt.Camera.look_at((0.1, 1.0, 2.3), (0.0, 1.0, 1.3), (0.0, 1.0, 0.0), 90.0)]
    rs, rc = (mrt.Renderer(A, W, H, 4, moments=True) for _ in range(2))
    ts, tc = Timer(hip, rs.stream()), Timer(hip, rc.stream())
    state = {"scene": 0, "cam": 0}

    def move(r, t, call):
        r.draw(1)
        r.sync()
        t0 = time.perf_counter()
        t.start()
        call()
        dev = t.stop_ms()
        r.sync()
        return dev, (time.perf_counter() - t0) * 1e3

    def move_scene():
        state["scene"] ^= 1
        return move(rs, ts, lambda: rs.move_scene((A, B)[state["scene"]]))

    def move_camera():
        state["cam"] ^= 1
        return move(rc, tc, lambda: rc.move_camera(C[state["cam"]]))

    for _ in range(2):   # the first moves allocate
        move_scene()
        move_camera()
    for k, v in alternate({"move_camera": move_camera, "move_scene": move_scene}, a.rounds).items():
        print(f"{name}: {k} device ms {fmt([d for d, _ in v])}; host ms to completion {fmt([h for _, h in v])} "
              f"(colour and moments)", flush=True)

    def set_scene():
        rs.draw(1)
        rs.sync()
        state["scene"] ^= 1
        t0 = time.perf_counter()
        rs.set_scene((A, B)[state["scene"]])
        return (time.perf_counter() - t0) * 1e3

    print(f"{name}: set_scene host ms {fmt([set_scene() for _ in range(a.rounds)])}", flush=True)
    rs.close()
    rc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--triangles", type=int, default=1 << 20)
    a = ap.parse_args()
    torch.zeros(1, device="cuda")
    mrt.device_count()
    hip = hip_runtime()
    print(f"{a.w}x{a.h}, fast build, {a.rounds} rounds", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        measure(a, hip, "cornellbox", mrt.Scene("cornellbox"),
                mrt.Scene(moved_cornellbox(tmp), mrt.scene_path("cornellbox")[:-4] + ".mtl"))
    big = [mrt.Scene("cornellbox", procedural_triangles=a.triangles, procedural_seed=s, bvh_builder=mrt.BVH_DEVICE_PLOC)
           for s in (1, 2)]
    measure(a, hip, f"cornellbox + {a.triangles} triangles", *big)


if __name__ == "__main__":
    main()
