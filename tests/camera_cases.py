"""Shared by the camera tests: the test cameras, a float64 model of the
camera-ray definition (include/mrt.h, DESIGN.md "Camera") and a replay of a
render from given camera rays through the oracle's stages.

The oracle has no camera parameter; it does expose the stages.  A frame f of
the reference is raygen, then L x {intersect, shade, intersect the shadow rays,
resolve}, then accumulate(f) (renderer/Renderer.mm:500-585), iteration i
reading the noise table of frame noise_frame_for(f, i): replay_render does
exactly that from whatever camera rays it is given."""
from __future__ import annotations

import numpy as np

from helpers import SEED

# cornellbox spans x in [-1, 1], y in [0, 2], z in [-1, 1], open at z = 1
# name: (eye, target, up, fov_x_degrees, lens_radius, focus_distance)
CAMERAS = {
    "A": ((0.6, 1.4, 2.0), (-0.2, 0.7, 0.0), (0.0, 1.0, 0.0), 60.0, 0.0, 0.0),    # all geometry in front
    "B": ((2.5, 1.0, 2.5), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.0, 0.0),     # outside: the outer side of a wall
    "C": ((0.0, 1.0, 0.2), (0.0, 0.3, -0.6), (0.0, 1.0, 0.0), 100.0, 0.0, 0.0),   # inside: triangles cross the camera plane
    "D": ((0.6, 1.4, 2.0), (-0.2, 0.7, 0.0), (0.3, 1.0, 0.1), 20.0, 0.0, 0.0),    # roll, narrow view
    "E": ((0.6, 1.4, 2.0), (-0.2, 0.7, 0.0), (0.0, 1.0, 0.0), 60.0, 0.05, 2.0),   # A with a thin lens
    "W": ((0.5, 1.2, 2.2), (0.0, 0.6, 0.4), (0.0, 1.0, 0.0), 55.0, 0.0, 0.0),     # the water scene's view
}


def camera(mrt_mod, name):
    eye, target, up, fov, lens, focus = CAMERAS[name]
    return mrt_mod.Camera.look_at(eye, target, up, fov, lens_radius=lens, focus_distance=focus)


def camera_args(cam):
    """The 13 floats tools/primary_check.cpp takes for a pinhole camera, as
    strings that round-trip the float32 values."""
    vals = list(cam.origin) + list(cam.right) + list(cam.up) + list(cam.forward) + [cam.tan_half_fov]
    return ["%.9g" % v for v in vals]


def model_rays(cam, W, H, noise):
    """(origin, direction), float64 [W*H, 3], of the definition evaluated in
    float64 from the float32 camera fields and noise table (ray i = y * W + x)."""
    T = np.asarray(noise, np.float32).reshape(64, 64, 4).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    ns = T[y % 64, x % 64]
    u = (ns[..., 0] * 2.0 - 1.0) / (W - 1) + (2.0 * x / (W - 1) - 1.0)
    v = (ns[..., 1] * 2.0 - 1.0) / (H - 1) + (2.0 * y / (H - 1) - 1.0) * (H / W)
    s = float(cam.tan_half_fov)
    origin = np.array(list(cam.origin), np.float64)
    right, up, fwd = (np.array(list(a), np.float64) for a in (cam.right, cam.up, cam.forward))
    c = np.stack([u * s, v * s, -np.ones_like(u)], -1)
    o = np.broadcast_to(origin, c.shape).copy()
    if cam.lens_radius > 0:
        ls = T[(y + 32) % 64, (x + 32) % 64]
        rad = float(cam.lens_radius) * np.sqrt(ls[..., 2])
        lx, ly = rad * np.cos(2.0 * np.pi * ls[..., 3]), rad * np.sin(2.0 * np.pi * ls[..., 3])
        p = c * float(cam.focus_distance)
        w = np.stack([p[..., 0] - lx, p[..., 1] - ly, p[..., 2]], -1)
        o = o + right * lx[..., None] + up * ly[..., None]
    else:
        w = c
    w = w / np.linalg.norm(w, axis=-1, keepdims=True)
    d = right * w[..., 0:1] + up * w[..., 1:2] + fwd * (-w[..., 2:3])
    return o.reshape(-1, 3), d.reshape(-1, 3)


def replay_render(oracle_mod, osc, W, H, L, frames, rays_of_frame, seed=SEED):
    """The image [H, W, 4] of `frames` frames whose camera rays are
    rays_of_frame(f) (oracle RAY_DTYPE records in raygen's state)."""
    img = np.zeros((H, W, 4), np.float32)
    for f in range(frames):
        # a byte copy: the stages update the records in place, and a field-wise
        # numpy copy would leave the records' padding undefined
        rays = np.frombuffer(bytearray(np.ascontiguousarray(rays_of_frame(f)).tobytes()), oracle_mod.RAY_DTYPE)
        srays = np.zeros(W * H, oracle_mod.SRAY_DTYPE)
        for i in range(L):
            noise = oracle_mod.noise_table(seed, oracle_mod.noise_frame_for(f, i))
            isect = osc.intersect(rays)
            osc.shade(W, H, f, L, noise, isect, rays, srays)
            oracle_mod.resolve(osc.intersect(srays), rays, srays)
        oracle_mod.accumulate(f, rays, img)
    return img
