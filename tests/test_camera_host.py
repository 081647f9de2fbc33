"""Host side of the movable camera (include/mrt.h mrt_camera): the default
camera, mrt_camera_look_at, mrt_camera_check, the oracle replay helper the GPU
tests compare against (tests/camera_cases.py), and the candidate lists of moved
cameras (csrc/primary.cpp, checked by tools/primary_check.cpp with a camera)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from camera_cases import CAMERAS, camera, camera_args, replay_render
from helpers import SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-renderer_amd", "csrc")
SCENES = os.path.join(ROOT, "metal-renderer_amd", "scenes")
ERR_INVALID = -1


def test_default_camera_is_the_reference(mrt_mod):
    c = mrt_mod.Camera.default()
    assert list(c.origin) == [0.0, 1.0, np.float32(2.35)]
    assert list(c.forward) == [0.0, 0.0, -1.0]
    assert list(c.up) == [0.0, 1.0, 0.0]
    assert list(c.right) == [1.0, 0.0, 0.0]
    assert c.tan_half_fov == 1.0 and c.lens_radius == 0.0
    c.check()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_look_at_basis(mrt_mod, name):
    eye, target, up, fov, lens, focus = CAMERAS[name]
    c = camera(mrt_mod, name)
    r, u, f = (np.array(list(a), np.float64) for a in (c.right, c.up, c.forward))
    for a in (r, u, f):
        assert abs(np.dot(a, a) - 1.0) <= 1e-6
    assert abs(np.dot(r, u)) <= 1e-6 and abs(np.dot(r, f)) <= 1e-6 and abs(np.dot(u, f)) <= 1e-6
    assert np.abs(np.cross(r, u) + f).max() <= 1e-6          # right-handed: right x up = -forward
    view = np.array(target, np.float64) - np.array(eye, np.float64)
    assert np.abs(f - view / np.linalg.norm(view)).max() <= 1e-6
    assert np.dot(u, np.array(up)) > 0
    assert list(c.origin) == [np.float32(v) for v in eye]
    assert abs(c.tan_half_fov - math.tan(math.radians(fov) / 2)) <= 1e-6 * max(1.0, c.tan_half_fov)
    assert (c.lens_radius, c.focus_distance) == (np.float32(lens), np.float32(focus))


def _bad_cameras(mrt_mod):
    def mod(**kw):
        c = camera(mrt_mod, "A")
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c
    a = camera(mrt_mod, "A")
    return {
        "nan origin": mod(origin=(1, float("nan"))),
        "inf tan": mod(tan_half_fov=float("inf")),
        "nan focus": mod(focus_distance=float("nan")),
        "not unit": mod(up=(1, a.up[1] * 1.001)),
        "not orthogonal": mod(right=(0, a.right[0] + 1e-3)),
        "left-handed": _flip(mrt_mod),
        "tan zero": mod(tan_half_fov=0.0),
        "tan negative": mod(tan_half_fov=-1.0),
        "lens negative": mod(lens_radius=-0.1),
        "lens without focus": mod(lens_radius=0.1, focus_distance=0.0),
        "lens with negative focus": mod(lens_radius=0.1, focus_distance=-2.0),
    }


def _flip(mrt_mod):
    c = camera(mrt_mod, "A")
    for k in range(3):
        c.forward[k] = -c.forward[k]   # orthonormal still, right x up = +forward
    return c


def test_camera_check_rejects(mrt_mod):
    L = mrt_mod.lib()
    camera(mrt_mod, "E").check()
    for what, cam in _bad_cameras(mrt_mod).items():
        rc = L.mrt_camera_check(ctypes.byref(cam))
        assert rc == ERR_INVALID, what
        assert L.mrt_last_error(), what
        with pytest.raises(mrt_mod.MrtError):
            cam.check()
    assert L.mrt_camera_check(None) == ERR_INVALID


@pytest.mark.parametrize("eye,target,up,fov", [
    ((1, 2, 3), (1, 2, 3), (0, 1, 0), 60.0),          # eye == target
    ((0, 0, 0), (0, 2, 0), (0, 1, 0), 60.0),          # up parallel to the view direction
    ((0, 0, 0), (0, -2, 0), (0, 1, 0), 60.0),         # ... antiparallel
    ((0, 0, 0), (0, 0, -1), (0, 0, 0), 60.0),         # zero up
    ((0, 0, 0), (0, 0, -1), (0, 1, 0), 0.0),
    ((0, 0, 0), (0, 0, -1), (0, 1, 0), 180.0),
    ((0, 0, 0), (0, 0, -1), (0, 1, 0), -30.0),
    ((0, 0, 0), (0, 0, -1), (0, 1, 0), float("nan")),
    ((0, float("inf"), 0), (0, 0, -1), (0, 1, 0), 60.0),
])
def test_look_at_rejects(mrt_mod, eye, target, up, fov):
    L = mrt_mod.lib()
    v3 = ctypes.c_float * 3
    out = mrt_mod.Camera()
    rc = L.mrt_camera_look_at(v3(*eye), v3(*target), v3(*up), fov, ctypes.byref(out))
    assert rc == ERR_INVALID
    assert L.mrt_last_error()


def test_replay_helper_equals_oracle_render(oracle_mod, mrt_mod):
    """The replay of the stages from oracle.raygen's rays is OracleScene.render,
    bit for bit: the helper itself adds nothing of its own."""
    W, H, L, frames = 48, 40, 4, 2
    osc = oracle_mod.OracleScene(mrt_mod.scene_path("cornellbox"))
    ref, _ = osc.render(W, H, L, SEED, frames, threads=4)
    got = replay_render(oracle_mod, osc, W, H, L, frames,
                        lambda f: oracle_mod.raygen(W, H, oracle_mod.noise_table(SEED, f)))
    assert got.tobytes() == ref.tobytes()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("primary_camera") / "primary_check")
    srcs = [os.path.join(ROOT, "tools", "primary_check.cpp")] + [os.path.join(CSRC, f + ".cpp")
                                                                   for f in ("scene", "bvh", "primary")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe] + srcs, check=True)
    return exe


def _check(checker, mrt_mod, scene, W, H, jitters, cap, fast, cam_name):
    out = subprocess.run([checker, os.path.join(SCENES, scene + ".obj"), str(W), str(H), str(jitters), "0", str(cap),
                          str(fast)] + camera_args(camera(mrt_mod, cam_name)), capture_output=True, text=True)
    print(cam_name, scene, W, H, "fast" if fast else "ieee", out.stdout.strip())
    words = out.stdout.split()
    assert words[:2] == ["violations", "0"] and out.returncode == 0, out.stdout + out.stderr
    return out.stdout, int(words[words.index("listed") + 1])


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("cam_name", ["A", "B", "D"])
@pytest.mark.parametrize("W,H,jitters,cap", [(97, 61, 16, 12), (2, 2, 64, 40)])
def test_moved_camera_lists_are_conservative(checker, mrt_mod, cam_name, W, H, jitters, cap, fast):
    text, listed = _check(checker, mrt_mod, "cornellbox", W, H, jitters, cap, fast, cam_name)
    if cam_name == "A" and (W, H) == (97, 61):
        assert listed > 0, text


@pytest.mark.parametrize("fast", [0, 1])
def test_moved_camera_lists_water(checker, mrt_mod, fast):
    _check(checker, mrt_mod, "CornellBox-Water-plastic", 64, 36, 2, 40, fast, "A")


@pytest.mark.parametrize("fast", [0, 1])
def test_camera_inside_the_box(checker, mrt_mod, fast):
    """Camera C: triangles cross the camera plane and go into every list (or
    no lists are built); never a violation."""
    text, listed = _check(checker, mrt_mod, "cornellbox", 97, 61, 16, 12, fast, "C")
    assert listed > 0 or "lists not built" in text, text


def test_checker_without_camera_is_unchanged(checker):
    """No trailing camera: the reference's camera, as before."""
    out = subprocess.run([checker, os.path.join(SCENES, "cornellbox.obj"), "97", "61", "4", "0", "12", "0"],
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[:2] == ["violations", "0"], out.stdout + out.stderr
    bad = subprocess.run([checker, os.path.join(SCENES, "cornellbox.obj"), "97", "61", "4", "0", "12", "0", "1.0"],
                         capture_output=True, text=True)
    assert bad.returncode == 2
