"""Variance-guided denoising on the device against the numpy model of its
definitions (tests/variance_model.py): the luminance moments a renderer with
MRT_FLAG_MOMENTS accumulates, the stage calls mrt_moments, mrt_variance and
mrt_denoise_variance on synthetic inputs, and the renderer layer
(mrt_renderer_denoise_variance, read_variance, the CLI's --denoise-variance)
against the stage pipeline.

The precise build's moments are compared bit for bit.  Everywhere else the
tolerance is the rule of test_gpu_denoise.py: four times the largest deviation
of the float32 model from the float64 model on the same inputs, computed and
printed per case."""
import math
import os
import subprocess

import numpy as np
import pytest

from camera_cases import camera
from denoise_model import NOT_FILTERABLE, words
from helpers import dev_ptr, from_dev, to_dev
from test_gpu_denoise import synthetic
from variance_model import moments_accumulate32, moments_accumulate64, moments_records, svgf_atrous, variance

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5
DIRECT, STAGED = 1, 2
PATHS = [DIRECT, STAGED]
W0, H0, L0 = 96, 64, 4


def _scene(mrt_mod, cache={}):
    if "s" not in cache:
        cache["s"] = mrt_mod.Scene("cornellbox")
    return cache["s"]


def status_of(mrt_mod, fn, *args, **kw):
    with pytest.raises(mrt_mod.MrtError) as e:
        fn(*args, **kw)
    return e.value.status


def within(name, got, m64, m32):
    """got within 4 x the float32 model's deviation from the float64 model (where that one is finite)."""
    fin = np.isfinite(m64)
    dev32 = np.abs(m32[fin].astype(np.float64) - m64[fin]).max() if fin.any() else 0.0
    err = np.abs(got[fin].astype(np.float64) - m64[fin]).max() if fin.any() else 0.0
    print(f"{name}: float32 model deviates {dev32:.3g}, tolerance {4.0 * dev32:.3g}, kernel error {err:.3g}")
    assert np.isfinite(got[fin]).all()
    assert err <= 4.0 * dev32


# ---- moments through the renderer --------------------------------------------
def five_frames(mrt_mod, precise, cache={}):
    """The path radiance of frames 0..4: a renderer without accumulation that draws one frame five times."""
    if precise not in cache:
        r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise, accumulate_image=False)
        frames = []
        for _ in range(5):
            r.draw(1)
            frames.append(r.read_image().reshape(-1, 4)[:, :3].copy())
        r.close()
        cache[precise] = frames
    return cache[precise]


def test_renderer_moments_precise(gpu, mrt_mod, oracle_mod):
    sc = _scene(mrt_mod)
    plain = mrt_mod.Renderer(sc, W0, H0, L0, precise=True)
    plain.draw(5)
    want_img = plain.read_image()
    assert status_of(mrt_mod, plain.read_moments) == ERR_STATE     # without the flag
    assert status_of(mrt_mod, plain.moments_ptr) == ERR_STATE
    assert status_of(mrt_mod, plain.denoise_variance) == ERR_STATE
    plain.close()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    r.draw(5)
    assert r.read_image().tobytes() == want_img.tobytes()           # the image is what it was without the flag
    m5 = r.read_moments()
    want = moments_accumulate32(oracle_mod, five_frames(mrt_mod, True)).reshape(H0, W0, 4)
    assert m5.tobytes() == want.tobytes()
    assert (m5[..., 2] == 0).all() and (m5[..., 3] == 1).all() and m5[..., 0].max() > 0.1
    assert r.moments_ptr()
    # the frame order is the image's: any split of the five frames gives the same bits
    r.reset()
    r.draw(2)
    r.draw(3)
    assert r.read_moments().tobytes() == m5.tobytes()
    r.reset()
    for _ in range(5):
        r.draw(1)
    assert r.read_moments().tobytes() == m5.tobytes()
    # reset and set_camera restart them
    r.reset()
    r.draw(1)
    one = moments_accumulate32(oracle_mod, five_frames(mrt_mod, True)[:1]).reshape(H0, W0, 4)
    assert r.read_moments().tobytes() == one.tobytes()
    r.draw(4)
    r.set_camera(mrt_mod.Camera.default())
    r.draw(1)
    assert r.read_moments().tobytes() == one.tobytes()
    r.resize(48, 40)
    r.draw(2)
    assert r.read_moments().shape == (40, 48, 4) and (r.read_moments()[..., 3] == 1).all()
    r.close()


def test_renderer_moments_fast(gpu, mrt_mod, oracle_mod):
    frames = five_frames(mrt_mod, False)
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, moments=True)
    r.draw(5)
    got = r.read_moments().reshape(-1, 4)
    r.close()
    m64, m32 = moments_accumulate64(frames), moments_accumulate32(oracle_mod, frames)
    within("renderer moments, fast build, 5 frames", got, m64, m32)


def test_moments_flag_combinations(gpu, mrt_mod):
    sc = _scene(mrt_mod)
    assert status_of(mrt_mod, mrt_mod.Renderer, sc, W0, H0, L0, moments=True, accumulate_image=False) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.Renderer, sc, W0, H0, L0, moments=True, shard_count=2) == ERR_INVALID


# ---- mrt_moments ---------------------------------------------------------------
@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("f", [0, 1, 7])
def test_moments_stage_call(gpu, mrt_mod, oracle_mod, f, precise):
    W, H = 53, 37
    rng = np.random.default_rng(100 + f)
    rays = np.zeros(W * H, oracle_mod.RAY_DTYPE)
    rays["radiance"][:, :3] = rng.uniform(0.0, 3.0, size=(W * H, 3)).astype(np.float32)
    rgb = np.ascontiguousarray(rays["radiance"][:, :3])
    start = rng.uniform(0.0, 4.0, size=(W * H, 4)).astype(np.float32)
    d_rays, d_m = to_dev(rays), to_dev(start)
    mrt_mod.moments(_scene(mrt_mod), W, H, f, dev_ptr(d_rays), dev_ptr(d_m), precise=precise)
    got = from_dev(d_m, np.float32).reshape(-1, 4)
    assert from_dev(d_rays, np.uint8).tobytes() == rays.tobytes()      # the rays are only read
    m32 = start.copy()
    oracle_mod.accumulate(f, moments_records(oracle_mod, rgb), m32)
    if precise:
        assert got.tobytes() == m32.tobytes()
        return
    c = moments_accumulate64([rgb])
    m64 = c if f == 0 else c + (start.astype(np.float64) - c) * (f / (f + 1.0))
    m64[:, 3] = 1.0
    within(f"mrt_moments f={f}, fast build", got, m64, m32)


# ---- mrt_variance ------------------------------------------------------------
COUNTS = (0.0, 1.0, 3.0, 4.0, 16.0, 37.5)


def synthetic_moments(W, H, seed):
    """Counted moments over synthetic()'s guide planes: mu1 ~ U(0, 2), mu2 = mu1^2 + U(0, 0.5), the
    count by horizontal band one of COUNTS, one NaN mu1 and one Inf mu2 inside the planar regions."""
    _, gn, gp = synthetic(W, H, seed)
    rng = np.random.default_rng(seed + 1)
    m = np.zeros((H, W, 4), np.float32)
    m[..., 0] = rng.uniform(0.0, 2.0, size=(H, W))
    m[..., 1] = m[..., 0] * m[..., 0] + rng.uniform(0.0, 0.5, size=(H, W)).astype(np.float32)
    m[..., 2] = rng.uniform(0.0, 1.0, size=(H, W))
    m[..., 3] = np.asarray(COUNTS, np.float32)[(np.arange(H) * len(COUNTS)) // H][:, None]
    if W >= 5:
        a, b = W // 4, W // 2
        m[H // 4, a // 2, 0] = np.nan
        m[min(H - 1, H // 4 + 1), (a + b) // 2, 1] = np.inf
    return m, gn, gp


def gpu_variance(mrt_mod, m, gn, gp, params):
    H, W = m.shape[:2]
    d = [to_dev(np.ascontiguousarray(v, np.float32)) for v in (m, gn, gp)]
    d_v = to_dev(np.full((H, W), -3.0, np.float32))
    mrt_mod.variance(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_v), W, H, params)
    assert from_dev(d[0], np.float32).tobytes() == m.tobytes()
    return from_dev(d_v, np.float32).reshape(H, W)


@pytest.mark.parametrize("W,H", [(53, 37), (33, 9), (5, 3), (1, 1)])
def test_variance_matches_model(gpu, mrt_mod, W, H):
    m, gn, gp = synthetic_moments(W, H, 2000 * W + H)
    p = mrt_mod.SvgfParams.default()
    got = gpu_variance(mrt_mod, m, gn, gp, p)
    m64, m32 = variance(m, gn, gp, p, np.float64), variance(m, gn, gp, p, np.float32)
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.isfinite(m64).all()
    filt = words(gn) < NOT_FILTERABLE
    assert (got[~filt] == 0).all()                                 # misses and lights: exactly 0
    within(f"mrt_variance {W}x{H}", got, m64, m32)
    if W >= 33:
        assert (got[filt] > 0).mean() > 0.5
        # both estimates are in play, and a larger min_frames moves pixels to the spatial one
        q = mrt_mod.SvgfParams.default()
        q.min_frames = 17
        assert gpu_variance(mrt_mod, m, gn, gp, q).tobytes() != got.tobytes()


def test_variance_argument_errors(gpu, mrt_mod):
    n = 53 * 37
    m, g1, g2 = (to_dev(np.zeros(n * 4, np.float32)) for _ in range(3))
    v = to_dev(np.zeros(n, np.float32))
    p = mrt_mod.SvgfParams.default()
    call = lambda *a: mrt_mod.variance(*a[:4], 53, 37, *a[4:])   # noqa: E731
    assert status_of(mrt_mod, call, dev_ptr(m), dev_ptr(g1), dev_ptr(g2), dev_ptr(v), None) == ERR_INVALID
    for k, t in enumerate((m, g1, g2)):
        args = [dev_ptr(m), dev_ptr(g1), dev_ptr(g2), dev_ptr(t) + 16, p]
        assert status_of(mrt_mod, call, *args) == ERR_INVALID, k
    bad = mrt_mod.SvgfParams.default()
    bad.min_frames = 1
    with pytest.raises(mrt_mod.MrtError, match="min_frames"):
        call(dev_ptr(m), dev_ptr(g1), dev_ptr(g2), dev_ptr(v), bad)
    call(dev_ptr(m), dev_ptr(g1), dev_ptr(g2), dev_ptr(v), p)


# ---- mrt_denoise_variance -----------------------------------------------------
def synthetic_filter_input(W, H, seed):
    """synthetic()'s image and guides, and a variance plane ~ U(0, 0.5) that is exactly 0 on region 1."""
    img, gn, gp = synthetic(W, H, seed)
    var = np.random.default_rng(seed + 2).uniform(0.0, 0.5, size=(H, W)).astype(np.float32)
    var[:, W // 4:W // 2] = 0.0
    return img, var, gn, gp


def gpu_svgf(mrt_mod, img, var, gn, gp, params, path, want_variance=True):
    H, W = img.shape[:2]
    d = [to_dev(np.ascontiguousarray(v, np.float32)) for v in (img, var, gn, gp)]
    d_out, d_scr = to_dev(np.full((H, W, 4), -7.0, np.float32)), to_dev(np.full((H, W, 4), -9.0, np.float32))
    d_var = to_dev(np.full((H, W), -5.0, np.float32))
    mrt_mod.debug_denoise_path(path)
    try:
        mrt_mod.denoise_variance(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d[3]), dev_ptr(d_out),
                                 dev_ptr(d_scr), dev_ptr(d_var) if want_variance else None, W, H, params)
    finally:
        mrt_mod.debug_denoise_path(0)
    assert from_dev(d[0], np.float32).tobytes() == np.ascontiguousarray(img).tobytes()   # the inputs are only read
    assert from_dev(d[1], np.float32).tobytes() == np.ascontiguousarray(var).tobytes()
    return from_dev(d_out, np.float32).reshape(H, W, 4), from_dev(d_var, np.float32).reshape(H, W)


def filter_models(img, var, gn, gp, params, cache={}):
    key = (img.tobytes(), var.tobytes(), bytes(params))
    if key not in cache:
        cache[key] = (svgf_atrous(img, var, gn, gp, params, np.float64), svgf_atrous(img, var, gn, gp, params, np.float32))
    return cache[key]


CASES = [(53, 37, n) for n in (1, 2, 3, 4, 5)] + [(33, 9, 3), (5, 3, 5), (1, 1, 2), (64, 64, 3)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("W,H,iterations", CASES)
def test_denoise_variance_matches_model(gpu, mrt_mod, W, H, iterations, path):
    img, var, gn, gp = synthetic_filter_input(W, H, 1000 * W + H)
    params = mrt_mod.SvgfParams(iterations, 4.0, 0.01, 6, 4)
    (c64, v64), (c32, v32) = filter_models(img, var, gn, gp, params)
    got, got_v = gpu_svgf(mrt_mod, img, var, gn, gp, params, path)
    fin = np.isfinite(c64).all(-1)
    filt = words(gn) < NOT_FILTERABLE
    assert got[~fin].tobytes() == img[~fin].tobytes()                 # an unrepairable pixel is kept
    assert got[~filt].tobytes() == img[~filt].tobytes()               # misses and lights: bit-identical
    assert got_v[~filt].tobytes() == var[~filt].tobytes()             # ... and they keep their variance
    assert got[..., 3].tobytes() == img[..., 3].tobytes()             # alpha
    if W >= 5:   # the non-finite pixels have usable neighbours: repaired
        assert fin.all() and not np.isfinite(img).all()
    within(f"colour {W}x{H} N={iterations} path {path}", got[..., :3], c64[..., :3], c32[..., :3])
    within(f"variance {W}x{H} N={iterations} path {path}", got_v, v64, v32)
    assert (got_v >= 0).all()
    if W > 1:
        ok = filt & np.isfinite(img).all(-1) & (var > 0)
        assert np.abs(got[ok][:, :3] - img[ok][:, :3]).max() > 1e-3   # it did filter
        assert got_v[ok].mean() < var[ok].mean()                      # and the variance went down
    # variance_out is optional, and the image does not depend on it
    alone, untouched = gpu_svgf(mrt_mod, img, var, gn, gp, params, path, want_variance=False)
    assert alone.tobytes() == got.tobytes() and (untouched == -5.0).all()


@pytest.mark.parametrize("path", PATHS)
def test_zero_iterations_copy_and_aliasing(gpu, mrt_mod, path):
    img, var, gn, gp = synthetic_filter_input(53, 37, 5)
    got, got_v = gpu_svgf(mrt_mod, img, var, gn, gp, mrt_mod.SvgfParams(0, 4.0, 0.01, 6, 4), path)
    assert got.tobytes() == img.tobytes() and got_v.tobytes() == var.tobytes()
    n = 53 * 37
    d = [to_dev(np.zeros(n * 4, np.float32)) for _ in range(5)]
    dv = [to_dev(np.zeros(n, np.float32)) for _ in range(2)]
    i, g1, g2, o, s = (dev_ptr(t) for t in d)
    v, vo = (dev_ptr(t) for t in dv)
    p = mrt_mod.SvgfParams.default()
    for args in [(i, v, g1, g2, i, s, vo), (i, v, g1, g2, o, i, vo), (i, v, g1, g2, o, o, vo),
                 (i, v, g1, g2, o + 16, o, vo), (i, v, o, g2, o, s, vo), (i, v, g1, s, o, s, vo),
                 (i, v, g1, g2, o, s, v), (i, v, g1, g2, o, s, v + 4), (i, v, g1, g2, o, s, o),
                 (i, v, g1, g2, o, s, i), (i, o, g1, g2, o, s, vo), (i, v, g1, g2, o, s, g1 + 64)]:
        assert status_of(mrt_mod, mrt_mod.denoise_variance, *args, 53, 37, p) == ERR_INVALID, args
    assert status_of(mrt_mod, mrt_mod.denoise_variance, i, v, g1, g2, o, s, vo, 53, 37, None) == ERR_INVALID
    for field, value in (("iterations", 9), ("sigma_luminance", 0.0), ("sigma_plane", float("nan")),
                         ("normal_log2_power", 9), ("min_frames", 1)):
        bad = mrt_mod.SvgfParams.default()
        setattr(bad, field, value)
        with pytest.raises(mrt_mod.MrtError, match=field):
            mrt_mod.denoise_variance(i, v, g1, g2, o, s, vo, 53, 37, bad)
    mrt_mod.denoise_variance(i, v, g1, g2, o, s, vo, 53, 37, p)


def test_paths_agree(gpu, mrt_mod):
    img, var, gn, gp = synthetic_filter_input(200, 120, 9)
    p = mrt_mod.SvgfParams(3, 4.0, 0.01, 6, 4)
    (a, av), (b, bv) = (gpu_svgf(mrt_mod, img, var, gn, gp, p, path) for path in (DIRECT, STAGED))
    assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-5 and np.abs(av - bv).max() <= 1e-5
    assert gpu_svgf(mrt_mod, img, var, gn, gp, p, 0)[0].tobytes() in (a.tobytes(), b.tobytes())


# ---- renderer layer ----------------------------------------------------------
class Stage:
    """The stage calls on device buffers of one size."""

    def __init__(self, mrt_mod, precise, W=W0, H=H0):
        self.m, self.precise, self.W, self.H = mrt_mod, precise, W, H

    def _buf(self, c=4):
        return to_dev(np.zeros((self.H, self.W, c), np.float32))

    def guides(self, cam):
        n, p = self._buf(), self._buf()
        self.m.guides(_scene(self.m), self.W, self.H, dev_ptr(n), dev_ptr(p), camera=cam, precise=self.precise)
        return n, p

    def resolve(self, img, frames, hist=None):
        d_img, out = to_dev(img), self._buf()
        self.m.temporal_resolve(dev_ptr(d_img), frames, dev_ptr(hist) if hist is not None else None, dev_ptr(out),
                                self.W, self.H)
        return out

    def reproject(self, prev, g_prev, cam_prev, g_cur):
        out = self._buf()
        self.m.reproject(dev_ptr(prev), dev_ptr(g_prev[0]), dev_ptr(g_prev[1]), cam_prev, dev_ptr(g_cur[0]),
                         dev_ptr(g_cur[1]), dev_ptr(out), self.W, self.H, self.m.ReprojectParams.default())
        return out

    def denoise_variance(self, resolved, moments, g, params):
        """(variance plane, denoised image) of the stage calls on resolved colour and moments."""
        var, out, scr = self._buf(1), self._buf(), self._buf()
        self.m.variance(dev_ptr(moments), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(var), self.W, self.H, params)
        self.m.denoise_variance(dev_ptr(resolved), dev_ptr(var), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(out),
                                dev_ptr(scr), None, self.W, self.H, params)
        return self.host(var, 1)[..., 0], self.host(out)

    def host(self, t, c=4):
        return from_dev(t, np.float32).reshape(self.H, self.W, c)


@pytest.mark.parametrize("precise", [True, False])
def test_renderer_denoise_variance_equals_stage_pipeline(gpu, mrt_mod, precise):
    st = Stage(mrt_mod, precise)
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    gA, gD = st.guides(A), st.guides(D)
    p = mrt_mod.SvgfParams.default()
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise, moments=True)
    assert status_of(mrt_mod, r.denoise_variance) == ERR_STATE        # nothing accumulated, no history
    assert status_of(mrt_mod, r.read_variance) == ERR_STATE
    r.set_camera(A)
    r.draw(4)
    r.denoise_variance()             # enqueued behind the draw, no sync in between
    den, var = r.read_denoised(), r.read_variance()
    img4, mom4 = r.read_image(), r.read_moments()
    res4, mres4 = st.resolve(img4, 4), st.resolve(mom4, 4)
    want_var, want = st.denoise_variance(res4, mres4, gA, p)
    assert den.tobytes() == want.tobytes() and var.tobytes() == want_var.tobytes()
    assert np.isfinite(den).all() and np.abs(den - img4).max() > 1e-3 and var.max() > 0
    assert r.read_resolved().tobytes() == st.host(res4).tobytes()
    plain = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    plain.set_camera(A)
    plain.draw(4)
    if precise:
        assert img4.tobytes() == plain.read_image().tobytes()         # the accumulation image is never written
    assert r.read_image().tobytes() == img4.tobytes()
    # the display of the denoised buffer
    flags = mrt_mod.DISPLAY_TONEMAP | mrt_mod.DISPLAY_SRGB
    d_den, d_out = to_dev(den), to_dev(np.zeros_like(den))
    mrt_mod.display(dev_ptr(d_den), dev_ptr(d_out), W0, H0, flags)
    assert r.display(mrt_mod.DISPLAY_DENOISED | flags).tobytes() == from_dev(d_out, np.float32).tobytes()
    # explicit parameters; a bad one is rejected by name
    q = mrt_mod.SvgfParams(2, 2.0, 0.02, 4, 8)
    r.denoise_variance(q)
    want_var, want = st.denoise_variance(res4, mres4, gA, q)
    assert r.read_denoised().tobytes() == want.tobytes() and r.read_variance().tobytes() == want_var.tobytes()
    with pytest.raises(mrt_mod.MrtError, match="sigma_luminance"):
        r.denoise_variance(mrt_mod.SvgfParams(2, -1.0, 0.02, 4, 8))
    # both histories follow a move
    r.move_camera(D)
    r.denoise_variance()             # no new frame: the pure reprojection, filtered
    hist, mhist = st.reproject(res4, gA, A, gD), st.reproject(mres4, gA, A, gD)
    zero = np.zeros((H0, W0, 4), np.float32)
    want_var, want = st.denoise_variance(st.resolve(zero, 0, hist), st.resolve(zero, 0, mhist), gD, p)
    assert r.read_denoised().tobytes() == want.tobytes()
    r.draw(2)
    r.denoise_variance()
    img2, mom2 = r.read_image(), r.read_moments()
    plain.move_camera(D)
    plain.draw(2)
    plain.resolve()
    if precise:
        assert img2.tobytes() == plain.read_image().tobytes()
    res, mres = st.resolve(img2, 2, hist), st.resolve(mom2, 2, mhist)
    assert r.read_resolved().tobytes() == st.host(res).tobytes()
    if precise:
        assert plain.read_resolved().tobytes() == st.host(res).tobytes()    # the move's colour result is what it was
    want_var, want = st.denoise_variance(res, mres, gD, p)
    assert r.read_denoised().tobytes() == want.tobytes() and r.read_variance().tobytes() == want_var.tobytes()
    assert abs(st.host(mres)[..., 3].max() - 6.0) < 1e-4
    plain.close()
    # set_camera drops both histories; resize drops the variance plane
    r.set_camera(A)
    assert status_of(mrt_mod, r.denoise_variance) == ERR_STATE
    r.draw(1)
    r.denoise_variance()
    want_var, want = st.denoise_variance(st.resolve(r.read_image(), 1), st.resolve(r.read_moments(), 1), gA, p)
    assert r.read_denoised().tobytes() == want.tobytes()
    r.resize(48, 40)
    assert status_of(mrt_mod, r.read_variance) == ERR_STATE
    r.draw(2)
    r.denoise_variance()
    assert r.read_variance().shape == (40, 48) and np.isfinite(r.read_denoised()).all()
    r.close()


def test_cli_denoise_variance(gpu, mrt_mod, tmp_path):
    """mrt_render --denoise-variance writes the variance-denoised image of the same render."""
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

    rgb = lambda a: np.ascontiguousarray(a[..., :3]).tobytes()   # noqa: E731
    r = mrt_mod.Renderer(_scene(mrt_mod), 64, 48, 4, precise=True, moments=True)
    r.draw(2)
    r.denoise_variance()
    want = r.read_denoised()
    assert run(["--denoise-variance"], "a.pfm").tobytes() == rgb(want)
    p = mrt_mod.SvgfParams.default()
    p.iterations, p.sigma_luminance = 2, 1.5
    r.denoise_variance(p)
    got = run(["--svgf-iterations", "2", "--svgf-sigma-luminance", "1.5"], "b.pfm")
    assert got.tobytes() == rgb(r.read_denoised()) and got.tobytes() != rgb(want)
    # with an orbit: after the last move's draw
    eye, target = ([float(np.float32(v)) for v in q] for q in ((0.0, 1.0, 2.35), (0.0, 1.0, 1.35)))
    for k in (1, 2):
        a = float(np.float32(5.0)) * k * (math.pi / 180.0)
        dx, dz = eye[0] - target[0], eye[2] - target[2]
        e = (target[0] + dx * math.cos(a) + dz * math.sin(a), eye[1], target[2] - dx * math.sin(a) + dz * math.cos(a))
        r.move_camera(mrt_mod.Camera.look_at(e, target, (0.0, 1.0, 0.0), 90.0))
        r.draw(2)
    r.denoise_variance()
    got = run(["--denoise-variance", "--orbit-steps", "2", "--orbit-degrees", "5"], "c.pfm")
    assert got.tobytes() == rgb(r.read_denoised())
    r.close()
    p = subprocess.run(base + ["--denoise-variance", "--denoise"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "exclude" in p.stderr
    p = subprocess.run(base + ["--denoise-variance", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "single rank" in p.stderr
