"""Host side of the temporal history: the reprojection parameters and their
check (libmrt, no device), identities of the numpy model of the two definitions
(tests/temporal_model.py) on analytic planar guides, the fragile share of every
case the GPU test compares (tests/temporal_cases.py), and the quality gate of
the definition on oracle renders across a camera move."""
import numpy as np
import pytest

from camera_cases import camera as cornell_camera, model_rays, replay_render
from denoise_model import NOT_FILTERABLE, guides_from_hits, rel_mse, words
from helpers import SEED
from temporal_cases import PAIRS, SIZES, case, counted_image, fragile_limit, raycast
from temporal_cases import camera as case_camera
from temporal_model import reproject, resolve


def test_default_params(mrt_mod):
    p = mrt_mod.ReprojectParams.default()
    assert p.plane_tolerance == np.float32(0.01)
    assert p.normal_cos_min == np.float32(0.9)
    assert p.max_history == 32.0
    p.check()
    mrt_mod.ReprojectParams(1e-6, -1.0, 0.0).check()     # the extremes of each range pass
    mrt_mod.ReprojectParams(10.0, 1.0, 1e6).check()


@pytest.mark.parametrize("field,value", [
    ("plane_tolerance", 0.0), ("plane_tolerance", -0.01), ("plane_tolerance", float("nan")),
    ("plane_tolerance", float("inf")),
    ("normal_cos_min", -1.5), ("normal_cos_min", 1.5), ("normal_cos_min", float("nan")),
    ("normal_cos_min", float("inf")),
    ("max_history", -1.0), ("max_history", float("nan")), ("max_history", float("inf")),
])
def test_check_rejects_bad_fields(mrt_mod, field, value):
    p = mrt_mod.ReprojectParams.default()
    setattr(p, field, value)
    with pytest.raises(mrt_mod.MrtError, match=field) as e:
        p.check()
    assert e.value.status == -1   # MRT_ERR_INVALID


def test_null_params_rejected(mrt_mod):
    assert mrt_mod.lib().mrt_reproject_params_check(None) == -1
    assert mrt_mod.lib().mrt_reproject_params_default(None) == -1


# ---- model identities --------------------------------------------------------
def test_resolve_branches():
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 2, (4, 6, 4)).astype(np.float32)
    hist = rng.uniform(0, 2, (4, 6, 4)).astype(np.float32)
    hist[..., 3] = rng.uniform(1, 30, (4, 6)).astype(np.float32)
    hist[0, 0] = 0.0
    img[1, 1, 2] = np.nan
    out = resolve(img, 4, hist)
    assert tuple(out[0, 0]) == tuple(img[0, 0, :3].astype(np.float64)) + (4.0,)      # no history
    assert out[1, 1].tobytes() == hist[1, 1].astype(np.float64).tobytes()            # repaired
    h, n = float(hist[2, 3, 3]), 4.0
    want = (h * hist[2, 3, :3].astype(np.float64) + n * img[2, 3, :3].astype(np.float64)) / (h + n)
    assert np.allclose(out[2, 3, :3], want, rtol=1e-15) and out[2, 3, 3] == h + n
    assert resolve(img, 0, hist)[2, 3].tobytes() == hist[2, 3].astype(np.float64).tobytes()   # no new frame
    none = resolve(img, 7, None)
    assert np.array_equal(none[..., 3], np.full((4, 6), 7.0)) and np.array_equal(none[2, :, :3], img[2, :, :3])


def test_same_camera_returns_prev(mrt_mod):
    W, H = 53, 37
    cam = case_camera(mrt_mod, "A")
    gn, gp = raycast(cam, W, H)
    prev = counted_image(W, H, 7)
    p = mrt_mod.ReprojectParams(0.01, 0.9, 64.0)
    out, fragile = reproject(prev, gn, gp, cam, gn, gp, p)
    filt = words(gn) < NOT_FILTERABLE
    usable = (prev[..., 3] > 0) & np.isfinite(prev[..., :3]).all(-1)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    sel = filt & inner & usable & ~fragile
    assert sel.sum() > 0.6 * W * H
    assert np.abs(out[sel] - prev[sel]).max() <= 1e-3          # the other taps' weights are ~1e-6
    assert not out[~filt].any()                                # misses and lights: no history
    assert fragile.sum() <= fragile_limit(W, H)
    # the cap
    capped, _ = reproject(prev, gn, gp, cam, gn, gp, mrt_mod.ReprojectParams(0.01, 0.9, 5.0))
    assert capped[..., 3].max() == 5.0 and np.abs(capped[sel][:, :3] - prev[sel][:, :3]).max() <= 1e-3


def test_camera_behind_gives_zero(mrt_mod):
    W, H = 53, 37
    prev, pn, pp, pcam, cn, cp = case(mrt_mod, "behind", W, H)
    out, fragile = reproject(prev, pn, pp, pcam, cn, cp, mrt_mod.ReprojectParams.default())
    assert not out.any() and not fragile.any()
    assert (words(cn) < NOT_FILTERABLE).mean() > 0.5


def test_one_pixel_pan_shifts_history(mrt_mod):
    """A plane facing the camera, seen by the same camera shifted sideways by
    exactly one pixel's footprint on the plane: the history is prev shifted by
    one pixel."""
    W, H, depth = 33, 17, 2.0
    cam = mrt_mod.Camera.default()
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    o = np.array(list(cam.origin), np.float64)
    step = 2.0 * depth / (W - 1)                       # one pixel on the plane z = o.z - depth (tan_half_fov 1)

    def guides(shift):
        px = o[0] + shift + (2.0 * x / (W - 1) - 1.0) * depth
        py = o[1] + (2.0 * y / (H - 1) - 1.0) * (H / W) * depth
        pos = np.stack([px, py, np.full_like(px, o[2] - depth)], -1)
        gn = np.zeros((H, W, 4), np.float32)
        gp = np.zeros((H, W, 4), np.float32)
        gn[..., 2] = 1.0
        gp[..., :3] = pos
        gp[..., 3] = np.linalg.norm(pos - (o + (shift, 0, 0)), axis=-1)
        return gn, gp

    rng = np.random.default_rng(11)
    prev = rng.uniform(0.1, 2.0, (H, W, 4)).astype(np.float32)
    (pn, pp), (cn, cp) = guides(0.0), guides(step)      # the current camera stands one pixel to the right
    out, fragile = reproject(prev, pn, pp, cam, cn, cp, mrt_mod.ReprojectParams(0.01, 0.9, 64.0))
    # current pixel x sees what the previous camera saw at x + 1
    assert np.abs(out[:, :-1] - prev[:, 1:]).max() <= 1e-3
    assert fragile.sum() <= H                           # at most the column that left the image


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("pair", [p[0] for p in PAIRS])
def test_gpu_cases_are_not_fragile(mrt_mod, pair, W, H):
    """The condition of tests/test_gpu_temporal.py on its own inputs, met by
    the model alone: the fragile share is at most 2 % of the pixels or 1 pixel."""
    prev, pn, pp, pcam, cn, cp = case(mrt_mod, pair, W, H)
    out, fragile = reproject(prev, pn, pp, pcam, cn, cp, mrt_mod.ReprojectParams.default())
    print(f"{pair} {W}x{H}: fragile {fragile.sum()} of {W * H}, history on {np.mean(out[..., 3] > 0):.3f}")
    assert fragile.sum() <= fragile_limit(W, H)
    if pair == "behind":
        assert not out.any()
    elif W >= 16:
        assert 0.2 < np.mean(out[..., 3] > 0) < 1.0      # the case carries history, and rejects some


# ---- quality gate ------------------------------------------------------------
def _camera_rays(oracle_mod, cam, W, H, noise):
    """raygen's records with the origin and direction of `cam` (float64 model
    of the camera-ray definition, camera_cases.model_rays)."""
    rays = oracle_mod.raygen(W, H, noise)
    o, d = model_rays(cam, W, H, noise)
    rays["origin"] = o.astype(np.float32)
    rays["direction"] = d.astype(np.float32)
    return rays


def _oracle_guides(oracle_mod, osc, cam, W, H):
    rays = _camera_rays(oracle_mod, cam, W, H, np.full(64 * 64 * 4, 0.5, np.float32))
    gn, gp = guides_from_hits(osc, osc.intersect(rays), rays)
    return gn.reshape(H, W, 4), gp.reshape(H, W, 4)


def test_model_quality_gate(mrt_mod, oracle_mod):
    """16 frames at the reference's camera, a move to a camera 0.1 to the
    right, 2 frames there: the resolved image is closer (relMSE, the formula of
    the denoiser's gate) to an independently seeded 256-frame render at the new
    camera than the 2-frame image alone.  Ratios resolved / image measured with
    this test (cornellbox 96x64, L = 4) for 1, 2 and 8 new frames:
    0.082 / 0.131 / 0.360 (DESIGN.md "Temporal reprojection")."""
    W, H, L = 96, 64, 4
    osc = oracle_mod.OracleScene(mrt_mod.scene_path("cornellbox"))
    old = mrt_mod.Camera.default()
    new = mrt_mod.Camera.look_at((0.1, 1.0, 2.35), (0.1, 1.0, 0.0), (0.0, 1.0, 0.0), 90.0)

    def render(cam, frames, seed):
        return replay_render(oracle_mod, osc, W, H, L, frames,
                             lambda f: _camera_rays(oracle_mod, cam, W, H, oracle_mod.noise_table(seed, f)), seed=seed)

    before = render(old, 16, SEED)
    pn, pp = _oracle_guides(oracle_mod, osc, old, W, H)
    cn, cp = _oracle_guides(oracle_mod, osc, new, W, H)
    hist, _ = reproject(resolve(before, 16), pn, pp, old, cn, cp, mrt_mod.ReprojectParams.default())
    filt = words(cn) < NOT_FILTERABLE
    share = float(np.mean(hist[..., 3][filt] > 0))
    print(f"history on {share:.4f} of the filterable pixels after the move")
    assert share > 0.8
    ref = render(new, 256, SEED + 1)
    ratios = {}
    for frames in (1, 2, 8):
        img = render(new, frames, SEED)
        out = resolve(img, frames, hist)
        assert np.isfinite(out).all()
        ratios[frames] = rel_mse(out, ref) / rel_mse(img, ref)
        print(f"cornellbox {W}x{H} L={L}, 16 frames carried, {frames} new: relMSE ratio {ratios[frames]:.3f}")
    assert ratios[2] < 1.0


def test_model_history_coverage_same_camera(mrt_mod, oracle_mod):
    """Condition of the GPU test's coverage check, on the model: cornellbox
    through camera A of camera_cases, moved to the same camera, keeps history
    on at least 0.9 of the filterable pixels (measured: 1.000)."""
    W, H = 64, 48
    osc = oracle_mod.OracleScene(mrt_mod.scene_path("cornellbox"))
    cam = cornell_camera(mrt_mod, "A")
    gn, gp = _oracle_guides(oracle_mod, osc, cam, W, H)
    prev = np.ones((H, W, 4), np.float32)
    hist, _ = reproject(prev, gn, gp, cam, gn, gp, mrt_mod.ReprojectParams.default())
    filt = words(gn) < NOT_FILTERABLE
    share = float(np.mean(hist[..., 3][filt] > 0))
    print(f"cornellbox camera A -> A {W}x{H}: history on {share:.4f} of the filterable pixels")
    assert share >= 0.9
