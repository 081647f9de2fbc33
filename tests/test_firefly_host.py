"""Host side of firefly suppression: the default parameters and their check
(libmrt, no device), hand-built cases of the definition's numpy model
(tests/firefly_model.py), the synthetic inputs of the GPU test with the share of
undecided pixels they give, and the quality gate of the definition — clamp +
variance-guided filter against the filter alone on oracle renders (DESIGN.md
§2.1s)."""
import numpy as np
import pytest

from denoise_model import NOT_FILTERABLE, rel_mse, words
from firefly_model import firefly_clamp, undecided
from helpers import host_threads
from test_denoise_host import oracle_guides
from test_gpu_denoise import synthetic
from variance_model import lum, moments_accumulate32, svgf_atrous, variance

IMAGE_SEED, REF_SEED, REF_FRAMES = 12345, 12346, 1024
SIZES = [(53, 37), (33, 9), (5, 3), (1, 1), (64, 64)]


class Params:
    """The defaults of mrt_firefly_params_default, for the model."""
    def __init__(self, radius=2, k=3.0, min_taps=3, normal_cos_min=0.9, plane_tolerance=0.01):
        self.radius, self.k, self.min_taps = radius, k, min_taps
        self.normal_cos_min, self.plane_tolerance = normal_cos_min, plane_tolerance


# ---- parameters ---------------------------------------------------
def test_default_params(mrt_mod):
    p = mrt_mod.FireflyParams.default()
    assert p.as_dict() == {"radius": 2, "k": 3.0, "min_taps": 3, "normal_cos_min": np.float32(0.9),
                           "plane_tolerance": np.float32(0.01)}
    p.check()


@pytest.mark.parametrize("field,value", [
    ("radius", 0), ("radius", 4), ("min_taps", 0),
    ("k", 0.0), ("k", -1.0), ("k", float("nan")), ("k", float("inf")),
    ("normal_cos_min", -1.5), ("normal_cos_min", 1.5), ("normal_cos_min", float("nan")),
    ("normal_cos_min", float("inf")),
    ("plane_tolerance", 0.0), ("plane_tolerance", -0.01), ("plane_tolerance", float("nan")),
    ("plane_tolerance", float("inf")),
])
def test_check_rejects_bad_fields(mrt_mod, field, value):
    p = mrt_mod.FireflyParams.default()
    setattr(p, field, value)
    with pytest.raises(mrt_mod.MrtError, match=field) as e:
        p.check()
    assert e.value.status == -1   # MRT_ERR_INVALID
    # the ends of each range pass
    mrt_mod.FireflyParams(1, 1e-6, 1, -1.0, 1e-6).check()
    mrt_mod.FireflyParams(3, 1e6, 0xFFFFFFFF, 1.0, 10.0).check()


def test_null_params_rejected(mrt_mod):
    assert mrt_mod.lib().mrt_firefly_params_check(None) == -1
    assert mrt_mod.lib().mrt_firefly_params_default(None) == -1


# ---- hand-built cases of the definition ----------------------------------------
def plane5(centre=40.0):
    """A 5x5 image of one plane (z = 0, word 0, t = 1): grey neighbours of known luminance, one bright centre."""
    rng = np.random.default_rng(11)
    img = np.ones((5, 5, 4), np.float32)
    g = rng.uniform(0.5, 1.5, size=(5, 5)).astype(np.float32)
    img[..., :3] = g[..., None]
    img[..., 3] = rng.uniform(0.0, 1.0, size=(5, 5)).astype(np.float32)
    img[2, 2, :3] = (centre, 0.5 * centre, 2.0 * centre)
    y, x = np.mgrid[0:5, 0:5].astype(np.float32)
    gn = np.zeros((5, 5, 4), np.float32)
    gp = np.zeros((5, 5, 4), np.float32)
    gn[..., 2] = 1.0
    gp[..., 0], gp[..., 1], gp[..., 3] = 0.1 * x, 0.1 * y, 1.0
    return img, gn, gp


def set_word(gn, where, word):
    w = words(gn).copy()
    w[where] = word
    gn[..., 3] = w.view(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bright_centre_is_clamped_to_the_cap(dtype):
    img, gn, gp = plane5()
    out, cap, mask, l = firefly_clamp(img, gn, gp, Params(), dtype)
    lq = np.delete(lum(img[..., :3], np.float64).reshape(-1), 12)          # the 24 neighbours
    want = lq.mean() + 3.0 * np.sqrt(max(0.0, (lq * lq).mean() - lq.mean() ** 2))
    assert mask.sum() == 1 and mask[2, 2]
    eps = 1e-12 if dtype is np.float64 else 1e-5
    assert abs(cap[2, 2] - want) <= eps * want
    assert abs(lum(out[2, 2, :3].astype(np.float32), np.float64) - want) <= max(eps, 1e-6) * want   # l(out) = cap
    assert np.allclose(out[2, 2, :3] / img[2, 2, :3], cap[2, 2] / l[2, 2], rtol=max(eps, 1e-7))  # the hue stays
    keep = ~mask
    assert out[keep].astype(np.float32).tobytes() == img[keep].tobytes()    # everything else bitwise
    assert out[2, 2, 3] == img[2, 2, 3]                                     # alpha copied
    # radius 1: the 8 nearest neighbours alone
    _, cap1, mask1, _ = firefly_clamp(img, gn, gp, Params(radius=1), dtype)
    l8 = np.delete(lum(img[1:4, 1:4, :3], np.float64).reshape(-1), 4)
    want1 = l8.mean() + 3.0 * np.sqrt(max(0.0, (l8 * l8).mean() - l8.mean() ** 2))
    assert mask1[2, 2] and abs(cap1[2, 2] - want1) <= eps * want1


def test_light_in_the_window_leaves_the_pixel():
    img, gn, gp = plane5()
    set_word(gn, (0, 4), 0x80000002)           # a light pixel in the window's corner
    out, _, mask, _ = firefly_clamp(img, gn, gp, Params(), np.float32)
    assert not mask[2, 2] and out.tobytes() == img.tobytes()
    assert not firefly_clamp(img, gn, gp, Params(radius=3), np.float32)[2][2, 2]
    assert firefly_clamp(img, gn, gp, Params(radius=1), np.float32)[2][2, 2]   # outside the 3x3 window
    set_word(gn, (0, 4), 0xFFFFFFFF)           # a miss is not a light
    assert firefly_clamp(img, gn, gp, Params(), np.float32)[2][2, 2]


@pytest.mark.parametrize("how", ["word", "normal", "plane", "nan-normal", "nan-colour"])
def test_too_few_counting_taps_leave_the_pixel(how):
    """All neighbours but two fail one tap condition: N = 2 < min_taps = 3 keeps the centre, min_taps = 2 clamps it."""
    img, gn, gp = plane5()
    other = np.ones((5, 5), bool)
    other[2, 2] = other[2, 1] = other[2, 3] = False
    if how == "word":
        set_word(gn, other, 5)
    elif how == "normal":
        gn[other, :3] = (0.0, 0.6, 0.8)        # n_p.n_q = 0.8 < 0.9
    elif how == "plane":
        gp[other, 2] = 0.02                    # |n_p.(x_q - x_p)| = 0.02 > 0.01 t_p
    elif how == "nan-normal":
        gn[other, 0] = np.nan
    else:
        img[other, 1] = np.nan
    out, _, mask, _ = firefly_clamp(img, gn, gp, Params(), np.float32)
    assert not mask[2, 2] and out[2, 2].tobytes() == img[2, 2].tobytes()
    out2, cap2, mask2, _ = firefly_clamp(img, gn, gp, Params(min_taps=2), np.float64)
    l2 = lum(img[2, [1, 3], :3], np.float64)
    want = l2.mean() + 3.0 * np.sqrt(max(0.0, (l2 * l2).mean() - l2.mean() ** 2))
    assert mask2[2, 2] and abs(cap2[2, 2] - want) <= 1e-12 * want


def test_black_neighbours_zero_the_centre():
    img, gn, gp = plane5()
    centre = img[2, 2].copy()
    img[..., :3] = 0.0
    img[2, 2] = centre
    out, cap, mask, _ = firefly_clamp(img, gn, gp, Params(), np.float32)
    assert mask[2, 2] and cap[2, 2] == 0.0
    assert (out[2, 2, :3] == 0.0).all() and out[2, 2, 3] == centre[3]


def test_non_finite_and_dark_centres_stay_bitwise():
    img, gn, gp = plane5()
    for value in (np.nan, np.inf):
        img[2, 2, 1] = value
        out, _, mask, _ = firefly_clamp(img, gn, gp, Params(), np.float32)
        assert not mask.any() and out.astype(np.float32).tobytes() == img.tobytes()
    img[2, 2, :3] = 0.0                        # l_p = 0: not eligible
    assert not firefly_clamp(img, gn, gp, Params(), np.float32)[2][2, 2]
    img[2, 2, :3] = 40.0
    set_word(gn, (2, 2), 0x80000001)           # the centre is a light pixel itself
    assert not firefly_clamp(img, gn, gp, Params(), np.float32)[2].any()


def test_single_pixel_image_is_unchanged():
    img = np.array([[[50.0, 60.0, 70.0, 0.25]]], np.float32)
    gn = np.array([[[0.0, 0.0, 1.0, 0.0]]], np.float32)
    gp = np.array([[[0.0, 0.0, 0.0, 1.0]]], np.float32)
    for R in (1, 2, 3):
        out, _, mask, _ = firefly_clamp(img, gn, gp, Params(radius=R), np.float32)
        assert not mask.any() and out.tobytes() == img.tobytes()


# ---- the GPU test's inputs -------------------------------------------------------
def planted(W, H, seed):
    """test_gpu_denoise's synthetic inputs with fireflies (50 times their
    neighbours' level) in the open, next to the light block, on a region border,
    in the image corner and beside the NaN pixel, as far as the size has room."""
    img, gn, gp = synthetic(W, H, seed)
    a, b, c = W // 4, W // 2, (3 * W) // 4
    spots = [(0, 0)]
    if W >= 5 and H >= 3:
        spots += [(H // 2, W - 1)]                    # the last column (region 3, the turning normals)
    if W >= 16 and H >= 8:
        spots += [((3 * H) // 4 - 1, (b + c) // 2),   # in the open (region 2)
                  (H // 2, a + 4),                    # two pixels from the light block: in the window from R = 2 on
                  ((3 * H) // 4 - 2, b),              # the first column of region 2
                  (H // 4, a // 2 + 1)]               # beside the NaN pixel
    for y, x in spots:
        if y < H and x < W and np.isfinite(img[y, x, :3]).all():
            img[y, x, :3] = 50.0 * np.maximum(img[y, x, :3], 0.5)
    return img, gn, gp


def model_pair(W, H, R, cache={}):
    """(inputs, float64 model, float32 model, tolerance, undecided mask) of one GPU case, computed once.
    The tolerance is four times the largest deviation of the float32 model from the float64 model, in the
    output and in the cap, over the pixels where the two decide alike."""
    if (W, H, R) not in cache:
        inputs = planted(W, H, 1000 * W + H)
        p = Params(radius=R)
        m64, m32 = firefly_clamp(*inputs, p, np.float64), firefly_clamp(*inputs, p, np.float32)
        agree = m64[2] == m32[2]
        fin = np.isfinite(m64[0]).all(-1) & agree
        dev = float(np.abs(m32[0][fin].astype(np.float64) - m64[0][fin]).max()) if fin.any() else 0.0
        capped = np.isfinite(m64[1]) & np.isfinite(m32[1])
        if capped.any():
            dev = max(dev, float(np.abs(m32[1][capped].astype(np.float64) - m64[1][capped]).max()))
        tol = 4.0 * dev
        cache[(W, H, R)] = (inputs, m64, m32, tol, undecided(m64[3], m64[1], tol))
    return cache[(W, H, R)]


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("W,H", SIZES)
def test_synthetic_inputs_decide_clearly(W, H, R):
    """On the GPU test's inputs the float32 model decides as the float64 model
    does outside the undecided pixels, which are at most 1 % of the filterable
    ones; the planted fireflies are clamped where the definition says so."""
    (img, gn, gp), m64, m32, tol, und = model_pair(W, H, R)
    filt = words(gn) < NOT_FILTERABLE
    print(f"{W}x{H} R={R}: tolerance {tol:.3g}, clamped {int(m64[2].sum())} of {int(filt.sum())} filterable, "
          f"undecided {int(und.sum())}")
    assert und.sum() <= 0.01 * filt.sum()
    assert np.array_equal(m64[2][~und], m32[2][~und])
    assert not m64[2][~filt].any()
    if W >= 5 and H >= 3:
        assert m64[2][H // 2, W - 1]                             # the last column
    if W >= 16 and H >= 8:
        a, b, c = W // 4, W // 2, (3 * W) // 4
        assert m64[2][(3 * H) // 4 - 1, (b + c) // 2]            # in the open
        assert m64[2][(3 * H) // 4 - 2, b]                       # on the border: its own region's taps suffice
        assert m64[2][H // 2, a + 4] == (R == 1)                 # the light block is in the window from R = 2 on
        if words(gn)[H // 4, a // 2 + 1] < NOT_FILTERABLE:
            assert m64[2][H // 4, a // 2 + 1]                    # beside the NaN pixel, which does not count
        assert m64[2].sum() >= 3


# ---- quality gate ----------------------------------------------------------------
def per_frame_radiance(oracle_mod, osc, W, H, L, frames):
    return [osc.render(W, H, L, IMAGE_SEED, 1, frame_begin=f, threads=host_threads(), flags=oracle_mod.NO_ACCUMULATE)[0]
            for f in range(frames)]


GATE = {"cornellbox": (1, 4, 16, 64), "CornellBox-Water": (1, 4, 16, 64)}


@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_model_quality_gate(mrt_mod, oracle_mod, scene):
    """relMSE of clamp + variance-guided filter over that of the filter alone,
    against an independently seeded 1024-frame reference (96x64, L = 4, seeds
    12345 / 12346, SvgfParams and FireflyParams defaults): on CornellBox-Water
    below 0.5 at 1 frame and below 1 at 4 and 16 frames; on cornellbox at most
    1.02 at 1, 16 and 64 frames.  Every ratio is printed."""
    W, H, L = 96, 64, 4
    osc = oracle_mod.OracleScene(mrt_mod.scene_path(scene))
    gn, gp = oracle_guides(oracle_mod, osc, W, H)
    ref, _ = osc.render(W, H, L, REF_SEED, REF_FRAMES, frame_begin=0, threads=host_threads())
    rad = per_frame_radiance(oracle_mod, osc, W, H, L, max(GATE[scene]))
    sp, fp = mrt_mod.SvgfParams.default(), mrt_mod.FireflyParams.default()
    ratio = {}
    for frames in GATE[scene]:
        img, _ = osc.render(W, H, L, IMAGE_SEED, frames, threads=host_threads())
        m = moments_accumulate32(oracle_mod, [r.reshape(-1, 4)[:, :3] for r in rad[:frames]]).reshape(H, W, 4).copy()
        m[..., 3] = frames
        v = variance(m, gn, gp, sp, np.float64).astype(np.float32)   # the clamp leaves the variance plane alone
        alone = svgf_atrous(img, v, gn, gp, sp, np.float64)[0]
        cl, _, mask, _ = firefly_clamp(img, gn, gp, fp, np.float32)
        both = svgf_atrous(cl.astype(np.float32), v, gn, gp, sp, np.float64)[0]
        e0, e1, e2 = rel_mse(img, ref), rel_mse(alone, ref), rel_mse(both, ref)
        ratio[frames] = e2 / e1
        print(f"{scene} {W}x{H} L={L} frames {frames}: relMSE undenoised {e0:.5f}, filter alone {e1:.5f}, "
              f"clamp + filter {e2:.5f} (ratio {e2 / e1:.3f}), clamped {int(mask.sum())} pixels "
              f"({100.0 * mask.mean():.2f} %), relMSE of the clamped image {rel_mse(cl, ref):.5f}")
        assert np.isfinite(both).all()
    if scene == "CornellBox-Water":
        assert ratio[1] < 0.5
        assert ratio[4] < 1.0 and ratio[16] < 1.0
    else:
        assert ratio[1] <= 1.02 and ratio[16] <= 1.02 and ratio[64] <= 1.02


# ---- calibration of the error estimate with the clamp on: measured, not asserted --
@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_calibration_with_the_clamp_is_measured(mrt_mod, oracle_mod, scene):
    """test_converge_host.py::test_calibration's E / truth (192x128, L = 4, eps =
    0.01, seeds 1 and 102, n = 8, 16, 32, 1024-frame reference) with the
    denoised denominator taken from clamp + filter, printed beside the filter
    alone.  No band is asserted: the stop rule's [0.6, 1.8] is a statement
    about the unclamped pipeline (DESIGN.md §2.1s holds the figures)."""
    from converge_model import tile_error, tile_threshold
    from test_converge_host import EPS, Frames, scene_setup

    osc, guides, l_ref = scene_setup(oracle_mod, mrt_mod, scene)
    sp, fp = mrt_mod.SvgfParams.default(), mrt_mod.FireflyParams.default()
    for seed in (1, 102):
        fr = Frames(oracle_mod, osc)
        for n in (8, 16, 32):
            while fr.n[0, 0] < n:
                fr.add(seed, int(fr.n[0, 0]))
            img = fr.image()
            v = variance(fr.moments(), guides[0], guides[1], sp, np.float64)
            cl, _, mask, _ = firefly_clamp(img, guides[0], guides[1], fp, np.float32)
            ratio = {}
            for name, src in (("off", img), ("on", cl.astype(np.float32))):
                den = svgf_atrous(src, v.astype(np.float32), guides[0], guides[1], sp, np.float64)[0].astype(np.float32)
                mean, pixels = tile_error(den, v, guides[0], EPS, np.float64)
                s = tile_threshold(mean, pixels, 0.0, len(mean), np.float64)[1]
                counted = (words(guides[0]) < NOT_FILTERABLE) & np.isfinite(img[..., :3]).all(-1)
                l = lum(img[..., :3], np.float64)
                truth = float((((l - l_ref) ** 2) / (l_ref ** 2 + EPS * EPS))[counted].mean())
                ratio[name] = float(s["frame_error"]) / truth
            print(f"{scene} seed {seed} n = {n}: E / truth with the filter alone {ratio['off']:.3f}, with clamp + "
                  f"filter {ratio['on']:.3f} ({int(mask.sum())} pixels clamped)")
            assert np.isfinite(ratio["on"]) and ratio["on"] > 0
