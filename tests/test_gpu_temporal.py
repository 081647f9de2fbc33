"""mrt_reproject and mrt_temporal_resolve against the float64 model of their
definitions (tests/temporal_model.py) on synthetic inputs
(tests/temporal_cases.py), and the renderer layer (mrt_renderer_move_camera,
_resolve, read_resolved, MRT_DISPLAY_RESOLVED, _denoise_resolved, the CLI's
--orbit-steps) against the stage pipeline mrt_guides x 2 + mrt_temporal_resolve
+ mrt_reproject + mrt_temporal_resolve.

Tolerance of the reproject comparison, on the pixels the model does not mark
fragile: four times the largest deviation of the float32 model from the float64
model on the same inputs (all four channels; the count channel, up to 32,
carries the largest), computed and printed per case.  Measured on an MI355X,
float32 model deviation / kernel error at 53x37, 64x64, 5x3, 2x2 (the tolerance
is four times the first):
  identical   1.91e-4 / 1.25e-4, 2.25e-4 / 2.15e-4, 3.15e-7 / 3.15e-7, 0 / 0   (fragile pixels 20, 23, 0, 0)
  translated  2.20e-4 / 2.20e-4, 1.78e-4 / 1.67e-4, 2.46e-6 / 2.56e-6, 3.29e-7 / 3.29e-7
  rotated     1.50e-4 / 1.53e-4, 2.01e-4 / 2.01e-4, 1.91e-6 / 1.94e-6, 7.44e-7 / 7.44e-7
  behind      0 / 0 at every size (all zeros)
  pan         1.70e-4 / 1.46e-4, 2.19e-4 / 1.68e-4, 1.27e-6 / 1.27e-6, 2.11e-7 / 2.11e-7
(no fragile pixel outside the identical pair).  Resolve: the blend deviates
2.06e-7 relative at 53x37, 9.4e-8 at 2x2 (bound 1e-6).  History coverage on
cornellbox A -> A: 1.0000 of the filterable pixels (DESIGN.md "Temporal
reprojection")."""
import math
import os
import subprocess

import numpy as np
import pytest

from camera_cases import camera
from denoise_model import NOT_FILTERABLE, words
from helpers import dev_ptr, from_dev, to_dev
from temporal_cases import PAIRS, SIZES, case, counted_image, fragile_limit
from temporal_model import reproject, resolve

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5


def status_of(mrt_mod, fn, *args):
    with pytest.raises(mrt_mod.MrtError) as e:
        fn(*args)
    return e.value.status


# ---- stage level -------------------------------------------------------------
def gpu_reproject(mrt_mod, prev, pn, pp, pcam, cn, cp, params):
    H, W = prev.shape[:2]
    hosts = [np.ascontiguousarray(v, np.float32) for v in (prev, pn, pp, cn, cp)]
    bufs = [to_dev(v) for v in hosts]
    d_out = to_dev(np.full((H, W, 4), -7.0, np.float32))
    p = [dev_ptr(b) for b in bufs]
    mrt_mod.reproject(p[0], p[1], p[2], pcam, p[3], p[4], dev_ptr(d_out), W, H, params)
    for b, v in zip(bufs, hosts):
        assert from_dev(b, np.float32).tobytes() == v.tobytes()   # the inputs are only read
    return from_dev(d_out, np.float32).reshape(H, W, 4)


def models(mrt_mod, pair, W, H, params, cache={}):
    key = (pair, W, H, bytes(params))
    if key not in cache:
        inputs = case(mrt_mod, pair, W, H)
        m64, fragile = reproject(*inputs, params, np.float64)
        m32, _ = reproject(*inputs, params, np.float32)
        cache[key] = (inputs, m64, m32, fragile)
    return cache[key]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("pair", [p[0] for p in PAIRS])
def test_reproject_matches_model(gpu, mrt_mod, pair, W, H):
    params = mrt_mod.ReprojectParams.default()
    inputs, m64, m32, fragile = models(mrt_mod, pair, W, H, params)
    assert fragile.sum() <= fragile_limit(W, H)             # a condition on the case, met by the model alone
    got = gpu_reproject(mrt_mod, *inputs, params)
    ok = ~fragile
    dev32 = np.abs(m32[ok].astype(np.float64) - m64[ok]).max()
    err = np.abs(got[ok].astype(np.float64) - m64[ok]).max()
    tol = 4.0 * dev32
    print(f"{pair} {W}x{H}: fragile {fragile.sum()}, history on {np.mean(got[..., 3] > 0):.3f}, float32 model deviates "
          f"{dev32:.3g}, tolerance {tol:.3g}, kernel error {err:.3g}")
    assert np.isfinite(got).all()
    assert (got[..., 3] >= 0).all() and (got[..., 3] <= params.max_history).all()
    none = got[..., 3] == 0
    assert not got[none].view(np.uint32).any()               # zero history is exactly (0, 0, 0, 0)
    assert not got[words(inputs[4]) >= NOT_FILTERABLE].view(np.uint32).any()
    assert np.array_equal(none[ok], m64[..., 3][ok] == 0)
    assert err <= tol
    if pair == "behind":
        assert not got.view(np.uint32).any()
    elif W >= 16:
        assert 0.2 < np.mean(~none) < 1.0


def test_reproject_argument_errors(gpu, mrt_mod):
    W, H = 8, 4
    d = [to_dev(np.zeros(W * H * 4, np.float32)) for _ in range(6)]
    p = [dev_ptr(t) for t in d]
    params = mrt_mod.ReprojectParams.default()
    mrt_mod.reproject(p[0], p[1], p[2], None, p[3], p[4], p[5], W, H, params)   # NULL camera = the default
    assert status_of(mrt_mod, mrt_mod.reproject, p[0], p[1], p[2], None, p[3], p[4], p[5], W, H, None) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.reproject, p[0], p[1], p[2], None, p[3], p[4], p[5], 1, 32, params) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.reproject, p[0], p[1], p[2], None, p[3], p[4], p[5], 32, 1, params) == ERR_INVALID
    for k in range(5):     # the output on top of each input, and overlapping it by one pixel
        assert status_of(mrt_mod, mrt_mod.reproject, p[0], p[1], p[2], None, p[3], p[4], p[k], W, H, params) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.reproject, p[0], p[1], p[2], None, p[3], p[4], p[0] + 16, W, H, params) == ERR_INVALID
    with pytest.raises(mrt_mod.MrtError, match="plane_tolerance"):
        mrt_mod.reproject(p[0], p[1], p[2], None, p[3], p[4], p[5], W, H, mrt_mod.ReprojectParams(0.0, 0.9, 32.0))


def gpu_resolve(mrt_mod, img, frames, hist):
    H, W = img.shape[:2]
    d_img, d_out = to_dev(img), to_dev(np.full((H, W, 4), -7.0, np.float32))
    d_hist = to_dev(hist) if hist is not None else None
    mrt_mod.temporal_resolve(dev_ptr(d_img), frames, dev_ptr(d_hist) if hist is not None else None, dev_ptr(d_out), W, H)
    assert from_dev(d_img, np.float32).tobytes() == img.tobytes()
    if hist is not None:
        assert from_dev(d_hist, np.float32).tobytes() == hist.tobytes()
    return from_dev(d_out, np.float32).reshape(H, W, 4)


@pytest.mark.parametrize("W,H", [(53, 37), (2, 2)])
def test_resolve(gpu, mrt_mod, W, H):
    """The three bitwise branches exactly; the blend within 1e-6 relative of
    the float64 model (at most four roundings of non-negative terms: two
    products or fused products, a sum, a quotient — 4 x 2^-24 = 2.4e-7)."""
    rng = np.random.default_rng(W)
    img = rng.uniform(0.01, 2.0, (H, W, 4)).astype(np.float32)
    hist = counted_image(W, H, 5) if W > 2 else rng.uniform(0.5, 9.0, (H, W, 4)).astype(np.float32)
    hist[~np.isfinite(hist).all(-1)] = 1.0
    hist[0, 0] = 0.0                       # no history here
    img[0, 1, 1] = np.nan                  # repaired by the history
    img[1, 0, 0] = np.inf
    has = hist[..., 3] > 0
    fin = np.isfinite(img[..., :3]).all(-1)
    assert has[0, 1] and has[1, 0] and not has[0, 0]
    got = gpu_resolve(mrt_mod, img, 3, hist)
    assert got[~has][:, :3].tobytes() == img[~has][:, :3].tobytes() and (got[~has][:, 3] == 3.0).all()
    assert got[has & ~fin].tobytes() == hist[has & ~fin].tobytes() and (has & ~fin).sum() == 2
    m64 = resolve(img, 3, hist)
    sel = has & fin
    rel = np.abs(got[sel].astype(np.float64) - m64[sel]) / np.abs(m64[sel])
    print(f"resolve {W}x{H}: blend deviates {rel.max():.3g} relative from the float64 model")
    assert rel.max() <= 1e-6
    assert np.array_equal(got[sel][:, 3], hist[sel][:, 3] + np.float32(3.0))
    # no new frame: the history, and the (uncounted) image where there is none
    got0 = gpu_resolve(mrt_mod, img, 0, hist)
    assert got0[has].tobytes() == hist[has].tobytes()
    assert got0[~has][:, :3].tobytes() == img[~has][:, :3].tobytes() and not got0[~has][:, 3].any()
    # no history: the image with its frame count
    gotn = gpu_resolve(mrt_mod, img, 7, None)
    assert gotn[..., :3].tobytes() == img[..., :3].tobytes() and (gotn[..., 3] == 7.0).all()
    d = [to_dev(np.zeros(W * H * 4, np.float32)) for _ in range(3)]
    i, h, o = (dev_ptr(t) for t in d)
    assert status_of(mrt_mod, mrt_mod.temporal_resolve, i, 1, h, i, W, H) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.temporal_resolve, i, 1, h, h, W, H) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.temporal_resolve, i, 1, None, i, W, H) == ERR_INVALID


# ---- renderer layer ----------------------------------------------------------
W0, H0, L0 = 64, 48, 4


def _scene(mrt_mod, cache={}):
    if "s" not in cache:
        cache["s"] = mrt_mod.Scene("cornellbox")
    return cache["s"]


def fresh_image(mrt_mod, cam, frames, precise, cache={}):
    """The image of a fresh renderer after set_camera(cam); draw(frames)."""
    key = (bytes(cam), frames, precise)
    if key not in cache:
        r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
        r.set_camera(cam)
        r.draw(frames)
        cache[key] = r.read_image()
        r.close()
    return cache[key]


class Stage:
    """The stage calls on device buffers of one size."""

    def __init__(self, mrt_mod, precise, W=W0, H=H0):
        self.m, self.precise, self.W, self.H = mrt_mod, precise, W, H

    def _buf(self):
        return to_dev(np.zeros((self.H, self.W, 4), np.float32))

    def guides(self, cam):
        n, p = self._buf(), self._buf()
        self.m.guides(_scene(self.m), self.W, self.H, dev_ptr(n), dev_ptr(p), camera=cam, precise=self.precise)
        return n, p

    def resolve(self, img, frames, hist=None):
        d_img, out = to_dev(img), self._buf()
        self.m.temporal_resolve(dev_ptr(d_img), frames, dev_ptr(hist) if hist is not None else None, dev_ptr(out),
                                self.W, self.H)
        return out

    def reproject(self, prev, g_prev, cam_prev, g_cur, params=None):
        out = self._buf()
        self.m.reproject(dev_ptr(prev), dev_ptr(g_prev[0]), dev_ptr(g_prev[1]), cam_prev, dev_ptr(g_cur[0]),
                         dev_ptr(g_cur[1]), dev_ptr(out), self.W, self.H, params or self.m.ReprojectParams.default())
        return out

    def host(self, t):
        return from_dev(t, np.float32).reshape(self.H, self.W, 4)


@pytest.mark.parametrize("precise", [True, False])
def test_move_camera_equals_stage_pipeline(gpu, mrt_mod, precise):
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    st = Stage(mrt_mod, precise)
    gA, gD = st.guides(A), st.guides(D)
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    r.set_camera(A)
    r.draw(4)
    r.move_camera(D)               # enqueued behind the draw, no sync in between
    r.draw(2)
    r.resolve()
    got, img = r.read_resolved(), r.read_image()
    assert img.tobytes() == fresh_image(mrt_mod, D, 2, precise).tobytes()     # the history lives beside the image
    hist = st.reproject(st.resolve(fresh_image(mrt_mod, A, 4, precise), 4), gA, A, gD)
    want = st.resolve(img, 2, hist)
    assert got.tobytes() == st.host(want).tobytes()
    assert np.isfinite(got).all() and np.mean(got[..., 3] > 2) > 0.3 and abs(got[..., 3].max() - 6.0) < 1e-4
    assert r.camera.as_dict() == D.as_dict()
    # a chain A -> D -> A
    r.move_camera(A)
    r.draw(3)
    r.resolve()
    got2, img2 = r.read_resolved(), r.read_image()
    assert img2.tobytes() == fresh_image(mrt_mod, A, 3, precise).tobytes()
    want2 = st.resolve(img2, 3, st.reproject(want, gD, D, gA))
    assert got2.tobytes() == st.host(want2).tobytes()
    assert abs(got2[..., 3].max() - 9.0) < 1e-4 and got2.tobytes() != got.tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_then_first_plain_denoise(gpu, mrt_mod, precise):
    """A renderer that moves before it has a denoised buffer: its first plain
    denoise filters with the new camera's guide planes, the resolve beside it is
    that of test_move_camera_equals_stage_pipeline, and the planes the next move
    takes as the previous ones are the new camera's."""
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    st = Stage(mrt_mod, precise)
    gA, gD = st.guides(A), st.guides(D)
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    r.set_camera(A)
    r.draw(4)
    r.move_camera(D)
    r.draw(2)
    r.denoise()                    # the renderer's first denoise of any kind
    r.resolve()
    den, got, img = r.read_denoised(), r.read_resolved(), r.read_image()
    assert img.tobytes() == fresh_image(mrt_mod, D, 2, precise).tobytes()
    d_img, out, scr = to_dev(img), st._buf(), st._buf()
    mrt_mod.denoise(dev_ptr(d_img), dev_ptr(gD[0]), dev_ptr(gD[1]), dev_ptr(out), dev_ptr(scr), W0, H0,
                    mrt_mod.DenoiseParams.default(2))
    assert den.tobytes() == st.host(out).tobytes() and np.abs(den - img).max() > 1e-3
    want = st.resolve(img, 2, st.reproject(st.resolve(fresh_image(mrt_mod, A, 4, precise), 4), gA, A, gD))
    assert got.tobytes() == st.host(want).tobytes()
    r.move_camera(A)
    r.draw(3)
    r.resolve()
    got2, img2 = r.read_resolved(), r.read_image()
    assert img2.tobytes() == fresh_image(mrt_mod, A, 3, precise).tobytes()
    want2 = st.resolve(img2, 3, st.reproject(want, gD, D, gA))
    assert got2.tobytes() == st.host(want2).tobytes()
    assert abs(got2[..., 3].max() - 9.0) < 1e-4
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_two_moves_without_a_draw(gpu, mrt_mod, precise):
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    st = Stage(mrt_mod, precise)
    gA, gD = st.guides(A), st.guides(D)
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    r.set_camera(A)
    r.draw(4)
    r.move_camera(D)
    r.move_camera(A)
    r.resolve()                    # the pure reprojection: no frame at the new camera yet
    got, img = r.read_resolved(), r.read_image()
    assert img.tobytes() == fresh_image(mrt_mod, A, 4, precise).tobytes()     # reset keeps the content until a draw
    h1 = st.reproject(st.resolve(img, 4), gA, A, gD)
    h2 = st.reproject(st.resolve(img, 0, h1), gD, D, gA)
    assert got.tobytes() == st.host(st.resolve(img, 0, h2)).tobytes()
    assert r.stats()["frame_index"] == 0 and np.mean(got[..., 3] > 0) > 0.03   # D sees a ninth of A's view
    r.draw(2)
    assert r.read_image().tobytes() == fresh_image(mrt_mod, A, 2, precise).tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_camera_on_a_fresh_renderer_is_set_camera(gpu, mrt_mod, precise):
    D = camera(mrt_mod, "D")
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    r.move_camera(D)
    assert status_of(mrt_mod, r.resolve) == ERR_STATE           # nothing accumulated, nothing carried
    r.draw(2)
    r.resolve()
    got, img = r.read_resolved(), r.read_image()
    assert img.tobytes() == fresh_image(mrt_mod, D, 2, precise).tobytes()
    assert got[..., :3].tobytes() == img[..., :3].tobytes() and (got[..., 3] == 2.0).all()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_set_camera_reset_resize_drop_the_history(gpu, mrt_mod, precise):
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)

    def carried():
        r.draw(3)
        r.move_camera(D)
        r.draw(1)
        r.resolve()
        assert r.read_resolved()[..., 3].max() > 3.5     # more than the one frame since the move

    def plain(frames):
        r.draw(frames)
        r.resolve()
        got, img = r.read_resolved(), r.read_image()
        assert got[..., :3].tobytes() == img[..., :3].tobytes() and (got[..., 3] == float(frames)).all()

    carried()
    r.set_camera(A)
    assert status_of(mrt_mod, r.resolve) == ERR_STATE
    plain(2)
    carried()
    r.reset()
    assert status_of(mrt_mod, r.resolve) == ERR_STATE
    plain(1)
    carried()
    r.resize(48, 40)
    assert status_of(mrt_mod, r.read_resolved) == ERR_STATE     # no resolve at the new size yet
    assert status_of(mrt_mod, r.resolve) == ERR_STATE
    plain(2)
    carried()                                                   # the buffers were re-made for the new size
    assert r.read_resolved().shape == (40, 48, 4)
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_state_and_argument_errors(gpu, mrt_mod, tmp_path, precise):
    sc, A = _scene(mrt_mod), camera(mrt_mod, "A")
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise)
    assert status_of(mrt_mod, r.resolve) == ERR_STATE
    assert status_of(mrt_mod, r.denoise_resolved) == ERR_STATE
    r.draw(2)
    assert status_of(mrt_mod, r.read_resolved) == ERR_STATE
    assert status_of(mrt_mod, r.save_resolved, str(tmp_path / "x.pfm")) == ERR_STATE
    assert status_of(mrt_mod, r.display, mrt_mod.DISPLAY_RESOLVED) == ERR_STATE
    assert status_of(mrt_mod, r.display_enqueue, 0, mrt_mod.DISPLAY_RESOLVED) == ERR_STATE
    # a failed move leaves the renderer, its image and its camera as they were
    before, cam0 = r.read_image(), r.camera.as_dict()
    with pytest.raises(mrt_mod.MrtError, match="plane_tolerance") as e:
        r.move_camera(A, mrt_mod.ReprojectParams(-1.0, 0.9, 32.0))
    assert e.value.status == ERR_INVALID
    bad = mrt_mod.Camera.default()
    bad.tan_half_fov = 0.0
    assert status_of(mrt_mod, r.move_camera, bad) == ERR_INVALID
    assert r.stats()["frame_index"] == 2 and r.camera.as_dict() == cam0
    assert r.read_image().tobytes() == before.tobytes()
    r.resolve()
    assert status_of(mrt_mod, r.display, mrt_mod.DISPLAY_RESOLVED | mrt_mod.DISPLAY_DENOISED) == ERR_INVALID
    r.save_resolved(str(tmp_path / "r.pfm"))
    with open(tmp_path / "r.pfm", "rb") as f:
        assert f.readline().strip() == b"PF"
        assert tuple(map(int, f.readline().split())) == (W0, H0)
        f.readline()
        pix = np.frombuffer(f.read(), "<f4").reshape(H0, W0, 3)
    assert pix.tobytes() == np.ascontiguousarray(r.read_resolved()[..., :3]).tobytes()
    r.close()
    # a sharded renderer keeps no history
    s = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise, shard_rank=0, shard_count=2)
    s.draw(1)
    assert status_of(mrt_mod, s.move_camera, A) == ERR_STATE
    assert status_of(mrt_mod, s.resolve) == ERR_STATE
    assert status_of(mrt_mod, s.denoise_resolved) == ERR_STATE
    assert s.stats()["frame_index"] == 1
    s.close()


@pytest.mark.parametrize("precise", [True, False])
def test_display_and_denoise_of_the_resolved_buffer(gpu, mrt_mod, precise):
    sc, A, D = _scene(mrt_mod), camera(mrt_mod, "A"), camera(mrt_mod, "D")
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise)
    r.set_camera(A)
    r.draw(4)
    r.move_camera(D)
    r.draw(2)
    r.resolve()
    res, img = r.read_resolved(), r.read_image()
    flags = mrt_mod.DISPLAY_TONEMAP | mrt_mod.DISPLAY_SRGB
    d_res, d_out = to_dev(res), to_dev(np.zeros_like(res))
    mrt_mod.display(dev_ptr(d_res), dev_ptr(d_out), W0, H0, flags)
    want = from_dev(d_out, np.float32).reshape(H0, W0, 4).copy()
    got = r.display(mrt_mod.DISPLAY_RESOLVED | flags)
    assert got.tobytes() == want.tobytes() and got.tobytes() != r.display(flags).tobytes()
    r.display_enqueue(1, mrt_mod.DISPLAY_RESOLVED | flags)
    assert r.display_map(1).tobytes() == want.tobytes()
    mrt_mod.display(dev_ptr(d_res), dev_ptr(d_out), W0, H0, flags | mrt_mod.DISPLAY_RESOLVED)   # the stage call ignores the bit
    assert from_dev(d_out, np.float32).tobytes() == want.tobytes()
    # denoise_resolved = resolve + mrt_denoise of the resolved buffer with the new camera's guides
    st = Stage(mrt_mod, precise)
    gD = st.guides(D)

    def filtered(params):
        out, scr = st._buf(), st._buf()
        mrt_mod.denoise(dev_ptr(d_res), dev_ptr(gD[0]), dev_ptr(gD[1]), dev_ptr(out), dev_ptr(scr), W0, H0, params)
        return st.host(out)

    r.denoise_resolved()
    den = r.read_denoised()
    assert den.tobytes() == filtered(mrt_mod.DenoiseParams.default(2)).tobytes()
    assert r.read_resolved().tobytes() == res.tobytes() and np.abs(den - res).max() > 1e-3
    p = mrt_mod.DenoiseParams(1, 0.5, 0.02, 4)
    r.denoise_resolved(p)
    assert r.read_denoised().tobytes() == filtered(p).tobytes()
    assert r.display(mrt_mod.DISPLAY_DENOISED).tobytes() != r.display(mrt_mod.DISPLAY_RESOLVED).tobytes()
    assert r.read_image().tobytes() == img.tobytes()          # never written
    r.denoise()                                               # the plain denoise still filters the image alone
    d_img, out, scr = to_dev(img), st._buf(), st._buf()
    mrt_mod.denoise(dev_ptr(d_img), dev_ptr(gD[0]), dev_ptr(gD[1]), dev_ptr(out), dev_ptr(scr), W0, H0,
                    mrt_mod.DenoiseParams.default(2))
    assert r.read_denoised().tobytes() == st.host(out).tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_history_coverage_same_camera(gpu, mrt_mod, precise):
    """Moved to the same camera, cornellbox through camera A keeps history on
    at least 0.9 of the filterable pixels (the model on the oracle's guides:
    1.000, tests/test_temporal_host.py)."""
    A = camera(mrt_mod, "A")
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise)
    r.set_camera(A)
    r.draw(1)
    r.move_camera(A)
    r.resolve()
    got = r.read_resolved()
    r.close()
    st = Stage(mrt_mod, precise)
    filt = words(st.host(st.guides(A)[0])) < NOT_FILTERABLE
    share = float(np.mean(got[..., 3][filt] > 0))
    print(f"cornellbox camera A -> A {W0}x{H0}: history on {share:.4f} of the filterable pixels")
    assert filt.mean() > 0.5 and share >= 0.9
    assert not got[..., 3][~filt].any()


@pytest.mark.parametrize("precise", [True, False])
def test_cli_orbit(gpu, mrt_mod, tmp_path, precise):
    """mrt_render --orbit-steps 2 --orbit-degrees 5 writes the resolved image
    of the same sequence through the binding."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    base = [exe, "--scene", "cornellbox", "--w", "64", "--h", "48", "--spp", "2", "--L", "4",
            "--orbit-steps", "2", "--orbit-degrees", "5"] + (["--precise"] if precise else [])

    def run(extra, name):
        out = tmp_path / name
        p = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF"
            w, h = map(int, f.readline().split())
            assert (w, h) == (64, 48) and float(f.readline()) < 0
            return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)

    # the CLI's defaults (the reference's view), which it holds as floats and turns in double
    eye, target = ([float(np.float32(v)) for v in p] for p in ((0.0, 1.0, 2.35), (0.0, 1.0, 1.35)))
    r = mrt_mod.Renderer(_scene(mrt_mod), 64, 48, 4, precise=precise)
    r.draw(2)
    for k in (1, 2):
        a = float(np.float32(5.0)) * k * (math.pi / 180.0)
        dx, dz = eye[0] - target[0], eye[2] - target[2]
        e = (target[0] + dx * math.cos(a) + dz * math.sin(a), eye[1], target[2] - dx * math.sin(a) + dz * math.cos(a))
        r.move_camera(mrt_mod.Camera.look_at(e, target, (0.0, 1.0, 0.0), 90.0))
        r.draw(2)
    r.resolve()
    want = r.read_resolved()
    assert abs(want[..., 3].max() - 6.0) < 1e-4
    assert run([], "a.pfm").tobytes() == np.ascontiguousarray(want[..., :3]).tobytes()
    r.denoise_resolved()
    assert run(["--denoise"], "b.pfm").tobytes() == np.ascontiguousarray(r.read_denoised()[..., :3]).tobytes()
    r.close()
    p = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "single rank" in p.stderr
    p = subprocess.run([exe, "--orbit-degrees", "5"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--orbit-steps" in p.stderr
