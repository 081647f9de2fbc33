"""Host side of sampling to a target error (include/mrt.h "adaptive sampling",
DESIGN.md §2.1r): the parameters and their check (libmrt, no device); the
numpy models of the estimate (tests/converge_model.py) on hand-built cases;
the calibration of the estimate against oracle renders, which
is why it is built on the denoised image; and the stop rule's loop through the
models."""
import ctypes

import numpy as np
import pytest

from adaptive_model import accumulate64, tile_mask, tiles_of
from converge_model import tile_error, tile_threshold
from helpers import SEED, host_threads
from test_denoise_host import oracle_guides
from variance_model import lum, svgf_atrous, variance

MISS = np.uint32(0xFFFFFFFF).view(np.float32)


# ---- parameters ------------------------------------------------------
def test_default_params(mrt_mod):
    p = mrt_mod.ConvergeParams.default()
    assert p.as_dict() == {"target_error": np.float32(1e-3), "frames_per_pass": 8, "max_passes": 64, "max_tiles": 0,
                           "max_tile_frames": 0, "luminance_floor": np.float32(0.01)}
    p.check()
    q = mrt_mod.ConvergeParams.default(target_error=0.5, max_tiles=3)
    assert q.target_error == 0.5 and q.max_tiles == 3 and q.frames_per_pass == 8
    with pytest.raises(TypeError):
        mrt_mod.ConvergeParams.default(tiles=3)


@pytest.mark.parametrize("field,value", [
    ("target_error", 0.0), ("target_error", -1e-3), ("target_error", float("nan")), ("target_error", float("inf")),
    ("frames_per_pass", 0), ("max_passes", 0),
    ("luminance_floor", 0.0), ("luminance_floor", -0.01), ("luminance_floor", float("nan")), ("luminance_floor", float("inf")),
])
def test_check_names_the_bad_field(mrt_mod, field, value):
    with pytest.raises(mrt_mod.MrtError, match=field) as e:
        mrt_mod.ConvergeParams.default(**{field: value}).check()
    assert e.value.status == -1   # MRT_ERR_INVALID


def test_check_accepts_the_edges_and_rejects_null(mrt_mod):
    mrt_mod.ConvergeParams.default(target_error=1e-30, frames_per_pass=1, max_passes=1, max_tiles=0xFFFFFFFF,
                                   max_tile_frames=2 ** 63, luminance_floor=1e-30).check()
    L = mrt_mod.lib()
    assert L.mrt_converge_params_check(None) == -1 and L.mrt_converge_params_default(None) == -1
    # null arguments of the calls that take a device or a renderer: rejected before either is touched
    p = mrt_mod.AdaptiveParams.default()
    assert L.mrt_tile_error(None, None, None, None, None, 8, 8, ctypes.byref(p), 0, None) == -1
    assert L.mrt_tile_threshold(None, None, 4, 0.0, 4, None, None, None) == -1
    s, res = mrt_mod.ErrorSummary(), mrt_mod.ConvergeResult()
    assert L.mrt_renderer_error(None, None, 0.0, 0.0, ctypes.byref(s)) == -1
    assert L.mrt_renderer_converge(None, None, ctypes.byref(res)) == -1
    assert L.mrt_renderer_read_tile_error(None, None, None, 0) == -1


# ---- the models on hand-built cases ---------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tile_error_model(dtype):
    W, H = 130, 70                                                     # 3 x 2 tiles, the last column 2 px, the top row 6 px
    img = np.zeros((H, W, 4), np.float32)
    img[..., :3] = 0.5
    var = np.full((H, W), 0.25, np.float32)
    gn = np.zeros((H, W, 4), np.float32)
    gn[:64, 64:128, 3] = MISS                                          # tile 1: no counted pixel
    gn[0, 0, 3] = np.uint32(0x80000003).view(np.float32)               # a light pixel in tile 0
    img[1, 1, 2] = np.inf                                              # a non-finite pixel in tile 0
    img[2, 2, 3] = np.nan                                              # (the fourth channel does not matter)
    var[64:, :64] = 0.5                                                # tile 3: twice the error
    eps = np.float32(0.01)
    mean, pixels = tile_error(img, var, gn, eps, dtype)
    assert mean.shape == (6,) and mean.dtype == dtype and pixels.dtype == np.uint32
    assert pixels.tolist() == [64 * 64 - 2, 0, 2 * 64, 64 * 6, 64 * 6, 2 * 6]
    l = float(lum(np.float32([0.5, 0.5, 0.5]), np.float64))
    term = 0.25 / (l * l + float(eps) * float(eps))
    want = term * np.array([1, 0, 1, 2, 1, 1], np.float64)             # a mean: the tile's size does not matter
    np.testing.assert_allclose(mean.astype(np.float64), want, rtol=1e-5 if dtype == np.float32 else 1e-7)
    assert mean[1] == 0


def test_tile_threshold_model():
    #               0    1    2     3    4       5    6    7
    e = np.array([2.0, 5.0, 2.0, -1.0, 5.0, np.nan, 2.0, 9.0], np.float32)   # ties, a negative mean, a NaN mean
    n = np.array([10, 20, 10, 10, 20, 10, 10, 0], np.uint32)                 # tile 7: no counted pixel, its mean ignored
    lst, s = tile_threshold(e, n, 2.0, 8)                                    # a key equal to the threshold is not above
    assert lst.tolist() == [1, 4] and lst.dtype == np.uint32
    assert (s["tiles_above"], s["tiles_listed"], s["tiles_counted"], s["pixels"]) == (2, 2, 7, 90)
    assert s["max_tile_error"] == 5.0
    assert s["frame_error"] == np.float32((3 * 2.0 * 10 + 2 * 5.0 * 20) / 90)
    lst, s = tile_threshold(e, n, 1.0, 8)
    assert lst.tolist() == [1, 4, 0, 2, 6] and s["tiles_above"] == 5
    lst, s = tile_threshold(e, n, 1.0, 3)                                    # A above max_count: the worst three
    assert lst.tolist() == [1, 4, 0] and (s["tiles_above"], s["tiles_listed"]) == (5, 3)
    lst, s = tile_threshold(e, n, 0.0, 8)                                    # key 0 is never above, even at threshold 0
    assert lst.tolist() == [1, 4, 0, 2, 6]
    lst, s = tile_threshold(e, n, 5.0, 8)
    assert lst.tolist() == [] and (s["tiles_above"], s["tiles_listed"]) == (0, 0)
    lst, s = tile_threshold(np.array([np.inf, 1.0], np.float32), np.array([0, 0], np.uint32), 0.5, 2)
    assert lst.tolist() == [] and s == {"frame_error": 0, "max_tile_error": 0, "tiles_above": 0, "tiles_listed": 0,
                                        "tiles_counted": 0, "pixels": 0}


# ---- oracle renders, shared by the calibration and the loop ------------------------
W0, H0, L0, EPS = 192, 128, 4, 0.01
REF_FRAMES = 1024


class Frames:
    """Per-pixel counted accumulation in float64 of oracle frames: the image, the luminance moments, the counts."""

    def __init__(self, oracle_mod, osc):
        self.o, self.osc = oracle_mod, osc
        self.c, self.m, self.n = np.zeros((H0, W0, 3)), np.zeros((H0, W0, 2)), np.zeros((H0, W0))

    def add(self, seed, frame, mask=None):
        rgb = self.osc.render(W0, H0, L0, seed, 1, frame_begin=frame, threads=host_threads(), pixel_mask=mask,
                              flags=self.o.NO_ACCUMULATE)[0][..., :3].astype(np.float64)
        sel = np.ones((H0, W0), bool) if mask is None else mask.astype(bool)
        l = lum(rgb.astype(np.float32), np.float64)
        self.c[sel] = accumulate64(self.c, rgb, self.n)[sel]
        self.m[sel] = accumulate64(self.m, np.stack([l, l * l], -1), self.n)[sel]
        self.n[sel] += 1

    def image(self):
        return np.concatenate([self.c, self.n[..., None]], -1).astype(np.float32)

    def moments(self):
        return np.concatenate([self.m, np.zeros((H0, W0, 1)), self.n[..., None]], -1).astype(np.float32)


def scene_setup(oracle_mod, mrt_mod, scene, cache={}):
    """(oracle scene, guide planes, luminance of the 1024-frame reference), once per scene."""
    if scene not in cache:
        osc = oracle_mod.OracleScene(mrt_mod.scene_path(scene))
        ref = osc.render(W0, H0, L0, SEED + 7, REF_FRAMES, threads=host_threads())[0]
        cache[scene] = (osc, oracle_guides(oracle_mod, osc, W0, H0), lum(ref[..., :3], np.float64))
    return cache[scene]


def estimate(mrt_mod, img, mom, guides, threshold):
    """One estimate as mrt_renderer_error makes it, in float64: (variance, denoised, mean, pixels, list, summary)."""
    sp = mrt_mod.SvgfParams.default()
    v = variance(mom, guides[0], guides[1], sp, np.float64)
    den = svgf_atrous(img, v.astype(np.float32), guides[0], guides[1], sp, np.float64)[0].astype(np.float32)
    mean, pixels = tile_error(den, v, guides[0], EPS, np.float64)
    lst, s = tile_threshold(mean, pixels, threshold, len(mean), np.float64)
    return v, den, mean, pixels, lst, s


@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_calibration(mrt_mod, oracle_mod, scene):
    """E / truth at n = 8, 16, 32 accumulated frames, 192x128, L = 4, eps = 0.01, seeds 1 and 102, against a
    1024-frame reference of another seed.  E = the frame's mean of v / (l^2 + eps^2) over the counted pixels,
    truth = the mean of (l_image - l_ref)^2 / (l_ref^2 + eps^2) over the same pixels.

    With l from the DENOISED image the ratio must lie in [0.6, 1.8] (measured for the issue: 0.76 to 1.45); on
    CornellBox-Water with l from the image itself it must lie below 0.6 (measured: 0.20 to 0.41), which is why
    the feature does not use it.  Measured with this test: see DESIGN.md §2.1r."""
    osc, guides, l_ref = scene_setup(oracle_mod, mrt_mod, scene)
    for seed in (1, 102):
        fr = Frames(oracle_mod, osc)
        for n in (8, 16, 32):
            while fr.n[0, 0] < n:
                fr.add(seed, int(fr.n[0, 0]))
            img = fr.image()
            v, den, mean, pixels, _, s = estimate(mrt_mod, img, fr.moments(), guides, 0.0)
            own_mean, own_pixels = tile_error(img, v, guides[0], EPS, np.float64)
            own = tile_threshold(own_mean, own_pixels, 0.0, len(own_mean), np.float64)[1]
            assert own["pixels"] == s["pixels"] > 0                      # the same pixels count either way
            counted = (guides[0][..., 3].view(np.uint32) < 0x80000000) & np.isfinite(img[..., :3]).all(-1)
            assert int(counted.sum()) == s["pixels"]
            l = lum(img[..., :3], np.float64)
            truth = float((((l - l_ref) ** 2) / (l_ref ** 2 + EPS * EPS))[counted].mean())
            r_den, r_own = float(s["frame_error"]) / truth, float(own["frame_error"]) / truth
            print(f"{scene} seed {seed} n = {n}: truth {truth:.5g}, E / truth with the denoised denominator "
                  f"{r_den:.3f}, with the image's own {r_own:.3f}")
            assert 0.6 <= r_den <= 1.8
            if scene == "CornellBox-Water":
                assert r_own < 0.6


def test_loop_in_the_model(mrt_mod, oracle_mod):
    """mrt_renderer_converge's loop through the models on cornellbox: 8 base frames, target = half of the first
    estimate's max_tile_error, 8 extra frames per pass of every tile above the target."""
    osc, guides, _ = scene_setup(oracle_mod, mrt_mod, "cornellbox")
    F, seed = 8, SEED
    fr = Frames(oracle_mod, osc)
    for f in range(8):
        fr.add(seed, f)
    first = estimate(mrt_mod, fr.image(), fr.moments(), guides, 0.0)
    target = 0.5 * float(first[5]["max_tile_error"])
    started_below = first[2] <= target
    assert started_below.any() and not started_below.all()
    e = passes = 0
    converged = False
    while passes <= 16:
        _, _, mean, pixels, lst, s = estimate(mrt_mod, fr.image(), fr.moments(), guides, target)
        print(f"pass {passes}: tile means {np.array2string(mean, precision=5)}, above {lst.tolist()}")
        if s["tiles_above"] == 0:
            converged = True
            break
        mask = tile_mask(W0, H0, lst)
        for _ in range(F):
            fr.add(seed ^ mrt_mod.REFINE_SEED_XOR, e, mask)
            e += 1
        passes += 1
    assert converged and passes >= 1
    assert (mean <= target).all()
    extra = [fr.n[tile_mask(W0, H0, [t]).astype(bool)] for t in range(len(mean))]
    per_tile = np.array([int(x.flat[0]) - 8 for x in extra])
    assert all((x == x.flat[0]).all() for x in extra)                    # whole tiles only
    assert (per_tile[started_below] == 0).all() and (per_tile[~started_below] >= F).all()
    assert tiles_of(W0, H0) == (3, 2)
