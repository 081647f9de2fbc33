"""mrt_denoise against the float64 model of its definition
(tests/denoise_model.py) on synthetic inputs, and the renderer layer
(mrt_renderer_denoise, read_denoised, MRT_DISPLAY_DENOISED, the CLI's
--denoise) against the stage pipeline mrt_guides + mrt_denoise.

Tolerance of the model comparison: four times the largest deviation of the
float32 model from the float64 model on the same inputs (the margin covers the
kernels' native exp and their fused sums), computed and printed per case.
Measured on an MI355X, both kernels alike: 53x37 with 1..5 iterations float32
model 0.96e-6 .. 2.05e-6 (tolerance 3.8e-6 .. 8.2e-6), kernels 0.84e-6 ..
1.89e-6; 33x9 2.6e-6 / 1.7e-6; 5x3 5.4e-7 / 5.6e-7; 64x64 without the colour
term 6.5e-7 / 5.8e-7; 1x1 has one tap, and with IEEE division nothing to
differ in: 0 / 0 (DESIGN.md "Denoised output")."""
import os
import subprocess

import numpy as np
import pytest

from camera_cases import camera
from denoise_model import NOT_FILTERABLE, atrous, words
from helpers import dev_ptr, from_dev, to_dev

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5
DIRECT, STAGED = 1, 2      # mrt_debug_denoise_path: the two implementations of an iteration
PATHS = [DIRECT, STAGED]   # the staged one serves steps 1, 2, 4 (the direct one above)


def synthetic(W, H, seed):
    """A seeded random image (alpha random too) over guide planes of four
    regions with their own material words — three planes and, on the right, a
    surface whose normal turns smoothly — with a strip of misses on top, a
    block of light pixels in the middle, one NaN and one Inf pixel inside the
    planar regions, and one pixel whose guide normal is NaN (as far as the size
    has room for them)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, size=(H, W, 4)).astype(np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    gn = np.zeros((H, W, 4), np.float32)
    gp = np.zeros((H, W, 4), np.float32)
    word = np.zeros((H, W), np.uint32)
    a, b, c = W // 4, W // 2, (3 * W) // 4
    # region 0: the plane y = 0
    gn[:, :a, :3] = (0.0, 1.0, 0.0)
    gp[:, :a, 0], gp[:, :a, 2], gp[:, :a, 3] = 0.02 * x[:, :a], 0.02 * y[:, :a], 1.0 + 0.01 * y[:, :a]
    # region 1: the plane z = -1
    gn[:, a:b, :3] = (0.0, 0.0, 1.0)
    gp[:, a:b, 0], gp[:, a:b, 1], gp[:, a:b, 2] = 0.02 * x[:, a:b], 0.02 * y[:, a:b], -1.0
    gp[:, a:b, 3] = 2.0 + 0.005 * x[:, a:b]
    word[:, a:b] = 1
    # region 2: the plane x = 1
    gn[:, b:c, :3] = (1.0, 0.0, 0.0)
    gp[:, b:c, 0], gp[:, b:c, 1], gp[:, b:c, 2] = 1.0, 0.02 * y[:, b:c], 0.02 * x[:, b:c]
    gp[:, b:c, 3] = 1.2 + 0.004 * (x[:, b:c] + y[:, b:c])
    word[:, b:c] = 2
    # region 3: a unit sphere's surface, the normal turning 0.05 rad per pixel
    ang = 0.05 * x[:, c:] + 0.03 * y[:, c:]
    n3 = np.stack([np.sin(ang), np.full_like(ang, 0.3), np.cos(ang)], -1)
    n3 /= np.linalg.norm(n3, axis=-1, keepdims=True)
    gn[:, c:, :3] = n3
    gp[:, c:, :3] = n3
    gp[:, c:, 3] = 1.5
    word[:, c:] = 3
    if H >= 8:     # a strip of misses
        word[H - 2:] = 0xFFFFFFFF
        gn[H - 2:, :, :3] = 0.0
        gp[H - 2:] = (0.0, 0.0, 0.0, -1.0)
    if H >= 8 and W >= 16:   # a block of light pixels across regions 0 and 1
        word[H // 2 - 2:H // 2 + 2, a - 3:a + 3] |= 0x80000000
        gn[H // 4 + 2, (b + c) // 2, 0] = np.nan   # a NaN guide normal: the pixel keeps its value, its taps weigh 0
    gn[..., 3] = word.view(np.float32)
    if W >= 5:     # non-finite pixels inside the planes, with usable neighbours
        img[H // 4, a // 2, 1] = np.nan
        img[min(H - 1, H // 4 + 1), (a + b) // 2, 0] = np.inf
    return img, gn, gp


def gpu_denoise(mrt_mod, img, gn, gp, params, path):
    H, W = img.shape[:2]
    bufs = [to_dev(np.ascontiguousarray(v, np.float32)) for v in (img, gn, gp)]
    d_out, d_scr = to_dev(np.full((H, W, 4), -7.0, np.float32)), to_dev(np.full((H, W, 4), -9.0, np.float32))
    mrt_mod.debug_denoise_path(path)
    try:
        mrt_mod.denoise(dev_ptr(bufs[0]), dev_ptr(bufs[1]), dev_ptr(bufs[2]), dev_ptr(d_out), dev_ptr(d_scr), W, H, params)
    finally:
        mrt_mod.debug_denoise_path(0)
    assert from_dev(bufs[0], np.float32).tobytes() == np.ascontiguousarray(img).tobytes()   # the image is only read
    return from_dev(d_out, np.float32).reshape(H, W, 4)


def models(img, gn, gp, params, cache={}):
    key = (img.tobytes(), gn.tobytes(), bytes(params))
    if key not in cache:
        cache[key] = (atrous(img, gn, gp, params, np.float64), atrous(img, gn, gp, params, np.float32))
    return cache[key]


CASES = ([(53, 37, n, 1.0) for n in (1, 2, 3, 4, 5)] +   # at step 16 most taps leave the image
         [(33, 9, 3, 1.0),                               # one column and one row past a 32x8 tile
          (5, 3, 5, 1.0),                                # every non-centre tap outside from step 4 on
          (1, 1, 2, 1.0),
          (64, 64, 3, 0.0)])                             # no colour term


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("W,H,iterations,sigma_color", CASES)
def test_denoise_matches_model(gpu, mrt_mod, W, H, iterations, sigma_color, path):
    img, gn, gp = synthetic(W, H, 1000 * W + H)
    params = mrt_mod.DenoiseParams(iterations, sigma_color, 0.01, 6)
    m64, m32 = models(img, gn, gp, params)
    got = gpu_denoise(mrt_mod, img, gn, gp, params, path)
    fin = np.isfinite(m64).all(-1)
    dev32 = np.abs(m32[fin].astype(np.float64) - m64[fin]).max()
    err = np.abs(got[fin].astype(np.float64) - m64[fin]).max()
    tol = 4.0 * dev32
    print(f"{W}x{H} N={iterations} sigma_c={sigma_color} path {path}: float32 model deviates {dev32:.3g}, "
          f"tolerance {tol:.3g}, kernel error {err:.3g}, non-finite model pixels {np.sum(~fin)}")
    filt = words(gn) < NOT_FILTERABLE
    assert np.isfinite(got[fin]).all()                                # no NaN where the model has none
    assert got[~fin].tobytes() == img[~fin].tobytes()                 # ... and elsewhere the pixel is kept
    assert got[~filt].tobytes() == img[~filt].tobytes()               # misses and lights: bit-identical
    assert got[..., 3].tobytes() == img[..., 3].tobytes()             # alpha
    if W >= 5:   # the non-finite pixels have usable neighbours: repaired, and changed
        assert fin.all() and not np.isfinite(img).all()
    assert err <= tol
    if W > 1:
        ok = filt & np.isfinite(img).all(-1)
        assert np.abs(got[ok][:, :3] - img[ok][:, :3]).max() > 1e-3   # it did filter


@pytest.mark.parametrize("path", PATHS)
def test_zero_iterations_copy_and_aliasing(gpu, mrt_mod, path):
    img, gn, gp = synthetic(53, 37, 5)
    got = gpu_denoise(mrt_mod, img, gn, gp, mrt_mod.DenoiseParams(0, 1.0, 0.01, 6), path)
    assert got.tobytes() == img.tobytes()
    n = 53 * 37 * 4
    d = [to_dev(np.zeros(n, np.float32)) for _ in range(5)]
    i, g1, g2, o, s = (dev_ptr(t) for t in d)
    p = mrt_mod.DenoiseParams.default(1)
    for args in [(i, g1, g2, i, s), (i, g1, g2, o, i), (i, g1, g2, o, o), (i, g1, g2, o + 16, o),
                 (i, o, g2, o, s), (i, g1, s, o, s)]:
        with pytest.raises(mrt_mod.MrtError) as e:
            mrt_mod.denoise(*args, 53, 37, p)
        assert e.value.status == ERR_INVALID
    with pytest.raises(mrt_mod.MrtError) as e:
        mrt_mod.denoise(i, g1, g2, o, s, 53, 37, None)
    assert e.value.status == ERR_INVALID
    bad = mrt_mod.DenoiseParams(9, 1.0, 0.01, 6)
    with pytest.raises(mrt_mod.MrtError, match="iterations"):
        mrt_mod.denoise(i, g1, g2, o, s, 53, 37, bad)


def test_paths_agree(gpu, mrt_mod):
    """The two implementations give the same image to rounding (they sum the
    same taps in the same order), at a size of many tiles."""
    img, gn, gp = synthetic(200, 120, 9)
    p = mrt_mod.DenoiseParams(3, 1.0, 0.01, 6)
    a, b = (gpu_denoise(mrt_mod, img, gn, gp, p, path) for path in (DIRECT, STAGED))
    assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-5
    assert gpu_denoise(mrt_mod, img, gn, gp, p, 0).tobytes() in (a.tobytes(), b.tobytes())


# ---- renderer layer ---------------------------------------------------------
W0, H0, L0 = 96, 64, 4


def _scene(mrt_mod, cache={}):
    if "s" not in cache:
        cache["s"] = mrt_mod.Scene("cornellbox")
    return cache["s"]


def stage_pipeline(mrt_mod, sc, img, params, cam=None):
    """mrt.guides + mrt.denoise on a host image (precise guides, as a precise renderer's)."""
    H, W = img.shape[:2]
    d_img = to_dev(img)
    d_n, d_p, d_out, d_scr = (to_dev(np.zeros((H, W, 4), np.float32)) for _ in range(4))
    mrt_mod.guides(sc, W, H, dev_ptr(d_n), dev_ptr(d_p), camera=cam, precise=True)
    mrt_mod.denoise(dev_ptr(d_img), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_out), dev_ptr(d_scr), W, H, params)
    return from_dev(d_out, np.float32).reshape(H, W, 4)


def test_renderer_denoise_equals_stage_pipeline(gpu, mrt_mod):
    sc = _scene(mrt_mod)
    plain = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    plain.draw(5)
    five = plain.read_image()
    plain.close()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    r.draw(3)
    r.denoise()                       # enqueued behind the draw, no sync in between
    den = r.read_denoised()
    img = r.read_image()
    want = stage_pipeline(mrt_mod, sc, img, mrt_mod.DenoiseParams.default(3))
    assert den.tobytes() == want.tobytes()
    assert np.isfinite(den).all() and np.abs(den - img).max() > 1e-3
    fresh = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    fresh.draw(3)
    assert img.tobytes() == fresh.read_image().tobytes()      # the image is not written
    fresh.close()
    # explicit parameters
    p = mrt_mod.DenoiseParams(1, 0.5, 0.02, 4)
    r.denoise(p)
    assert r.read_denoised().tobytes() == stage_pipeline(mrt_mod, sc, img, p).tobytes()
    r.draw(2)
    assert r.read_image().tobytes() == five.tobytes()         # accumulation goes on as without a denoise
    r.close()


def test_renderer_guides_follow_camera_and_size(gpu, mrt_mod):
    sc, cam = _scene(mrt_mod), camera(mrt_mod, "A")
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    r.draw(3)
    r.denoise()
    before = r.read_denoised()
    r.set_camera(cam)
    r.draw(3)
    r.denoise()
    img = r.read_image()
    want = stage_pipeline(mrt_mod, sc, img, mrt_mod.DenoiseParams.default(3), cam)
    stale = stage_pipeline(mrt_mod, sc, img, mrt_mod.DenoiseParams.default(3), None)
    got = r.read_denoised()
    assert got.tobytes() == want.tobytes() and got.tobytes() != stale.tobytes() and got.tobytes() != before.tobytes()
    r.resize(48, 40)
    with pytest.raises(mrt_mod.MrtError) as e:     # no denoise at the new size yet
        r.read_denoised()
    assert e.value.status == ERR_STATE
    r.draw(2)
    r.denoise()
    img = r.read_image()
    assert img.shape == (40, 48, 4)
    want = stage_pipeline(mrt_mod, sc, img, mrt_mod.DenoiseParams.default(2), cam)
    assert r.read_denoised().tobytes() == want.tobytes()
    r.close()


def test_display_of_the_denoised_buffer(gpu, mrt_mod):
    sc = _scene(mrt_mod)
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    r.draw(3)
    r.denoise()
    den, img = r.read_denoised(), r.read_image()
    flags = mrt_mod.DISPLAY_TONEMAP | mrt_mod.DISPLAY_SRGB
    d_den, d_out = to_dev(den), to_dev(np.zeros_like(den))
    mrt_mod.display(dev_ptr(d_den), dev_ptr(d_out), W0, H0, flags)
    want = from_dev(d_out, np.float32).reshape(H0, W0, 4)
    got = r.display(mrt_mod.DISPLAY_DENOISED | flags)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != r.display(flags).tobytes()
    r.display_enqueue(1, mrt_mod.DISPLAY_DENOISED | flags)
    assert r.display_map(1).tobytes() == want.tobytes()
    # the stage call ignores the bit
    mrt_mod.display(dev_ptr(d_den), dev_ptr(d_out), W0, H0, flags | mrt_mod.DISPLAY_DENOISED)
    assert from_dev(d_out, np.float32).tobytes() == want.tobytes()
    assert r.read_image().tobytes() == img.tobytes()
    r.close()


def test_renderer_state_errors(gpu, mrt_mod, tmp_path):
    sc = _scene(mrt_mod)
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)

    def state_error(fn, *args):
        with pytest.raises(mrt_mod.MrtError) as e:
            fn(*args)
        assert e.value.status == ERR_STATE, e.value

    state_error(r.denoise)                                     # before any draw
    r.draw(1)
    state_error(r.read_denoised)                               # without a denoise
    state_error(r.save_denoised, str(tmp_path / "x.pfm"))
    state_error(r.display, mrt_mod.DISPLAY_DENOISED)
    state_error(r.display_enqueue, 0, mrt_mod.DISPLAY_DENOISED)
    r.denoise()
    r.read_denoised()
    r.reset()
    state_error(r.denoise)                                     # after reset
    r.set_camera(camera(mrt_mod, "A"))
    state_error(r.denoise)                                     # after set_camera
    r.draw(1)
    r.denoise()
    with pytest.raises(mrt_mod.MrtError, match="sigma_plane"):
        r.denoise(mrt_mod.DenoiseParams(1, 1.0, 0.0, 6))
    r.save_denoised(str(tmp_path / "d.pfm"))
    with open(tmp_path / "d.pfm", "rb") as f:
        assert f.readline().strip() == b"PF"
        assert tuple(map(int, f.readline().split())) == (W0, H0)
        f.readline()
        pix = np.frombuffer(f.read(), "<f4").reshape(H0, W0, 3)
    assert pix.tobytes() == np.ascontiguousarray(r.read_denoised()[..., :3]).tobytes()
    r.close()


def test_cli_denoise(gpu, mrt_mod, tmp_path):
    """mrt_render --denoise writes the denoised image of the same render."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    base = [exe, "--scene", "cornellbox", "--w", "64", "--h", "48", "--spp", "2", "--L", "4", "--precise"]

    def run(extra, name):
        out = tmp_path / name
        p = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF"
            w, h = map(int, f.readline().split())
            assert (w, h) == (64, 48) and float(f.readline()) < 0
            return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)

    r = mrt_mod.Renderer(_scene(mrt_mod), 64, 48, 4, precise=True)
    r.draw(2)
    r.denoise()
    want = r.read_denoised()
    assert run(["--denoise"], "a.pfm").tobytes() == np.ascontiguousarray(want[..., :3]).tobytes()
    p = mrt_mod.DenoiseParams.default(2)
    p.iterations, p.sigma_color = 1, 0.75
    r.denoise(p)
    got = run(["--denoise-iterations", "1", "--denoise-sigma-color", "0.75"], "b.pfm")
    assert got.tobytes() == np.ascontiguousarray(r.read_denoised()[..., :3]).tobytes()
    assert got.tobytes() != np.ascontiguousarray(want[..., :3]).tobytes()
    r.close()
