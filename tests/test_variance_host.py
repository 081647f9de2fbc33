"""Host side of variance-guided denoising: the default parameters and their
check (libmrt, no device), the model's temporal estimate against numpy's sample
variance, and the quality gate of the definitions — the numpy model
(tests/variance_model.py) on oracle renders, moments from the model's
recurrence over the oracle's per-frame radiance."""
import numpy as np
import pytest

from denoise_model import NOT_FILTERABLE, atrous, rel_mse, words
from helpers import SEED, host_threads
from test_denoise_host import oracle_guides
from variance_model import lum, moments_accumulate32, svgf_atrous, variance


def test_default_params(mrt_mod):
    p = mrt_mod.SvgfParams.default()
    assert p.as_dict() == {"iterations": 5, "sigma_luminance": 4.0, "sigma_plane": np.float32(0.01),
                           "normal_log2_power": 6, "min_frames": 4}
    p.check()


@pytest.mark.parametrize("field,value", [
    ("iterations", 9), ("normal_log2_power", 9), ("min_frames", 0), ("min_frames", 1),
    ("sigma_luminance", 0.0), ("sigma_luminance", -1.0), ("sigma_luminance", float("nan")),
    ("sigma_luminance", float("inf")),
    ("sigma_plane", 0.0), ("sigma_plane", -0.01), ("sigma_plane", float("nan")), ("sigma_plane", float("inf")),
])
def test_check_rejects_bad_fields(mrt_mod, field, value):
    p = mrt_mod.SvgfParams.default()
    setattr(p, field, value)
    with pytest.raises(mrt_mod.MrtError, match=field) as e:
        p.check()
    assert e.value.status == -1   # MRT_ERR_INVALID
    # the ends of each range pass
    mrt_mod.SvgfParams(8, 1e-6, 1e-6, 8, 2).check()
    mrt_mod.SvgfParams(0, 1e6, 10.0, 0, 0xFFFFFFFF).check()


def test_null_params_rejected(mrt_mod):
    assert mrt_mod.lib().mrt_svgf_params_check(None) == -1
    assert mrt_mod.lib().mrt_svgf_params_default(None) == -1


def test_temporal_estimate_is_the_sample_variance_of_the_mean():
    """k >= min_frames samples per pixel: max(0, mu2 - mu1^2) / (k - 1) == var(l, ddof=1) / k."""
    rng = np.random.default_rng(3)
    H, W, k = 5, 7, 9
    l = rng.uniform(0.0, 2.0, size=(k, H, W))
    m = np.zeros((H, W, 4))
    m[..., 0], m[..., 1], m[..., 3] = l.mean(0), (l * l).mean(0), k
    gn, gp = np.zeros((H, W, 4), np.float32), np.ones((H, W, 4), np.float32)
    gn[..., 2] = 1.0   # one plane, word 0

    class P:
        sigma_plane, normal_log2_power, min_frames = 0.01, 6, 4

    got = variance(m, gn, gp, P, np.float64)   # float64 moments: the definition's own arithmetic
    want = np.var(l, axis=0, ddof=1) / k
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def per_frame_radiance(oracle_mod, osc, W, H, L, frames):
    return [osc.render(W, H, L, SEED, 1, frame_begin=f, threads=host_threads(), flags=oracle_mod.NO_ACCUMULATE)[0]
            for f in range(frames)]


@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_model_quality_gate(mrt_mod, oracle_mod, scene):
    """Variance-guided relMSE < undenoised relMSE against an independently
    seeded 256-frame reference, for 1, 4 and 16 accumulated frames with
    SvgfParams.default().  Ratios denoised / undenoised (96x64, L = 4) are
    printed with the existing filter's beside them."""
    W, H, L = 96, 64, 4
    osc = oracle_mod.OracleScene(mrt_mod.scene_path(scene))
    gn, gp = oracle_guides(oracle_mod, osc, W, H)
    w = words(gn)
    assert (w < NOT_FILTERABLE).mean() > 0.5 and (w >= NOT_FILTERABLE).any()
    ref, _ = osc.render(W, H, L, SEED + 1, 256, frame_begin=0, threads=host_threads())
    rad = per_frame_radiance(oracle_mod, osc, W, H, L, 16)
    p = mrt_mod.SvgfParams.default()
    for frames in (1, 4, 16):
        img, _ = osc.render(W, H, L, SEED, frames, threads=host_threads())
        m = moments_accumulate32(oracle_mod, [r.reshape(-1, 4)[:, :3] for r in rad[:frames]]).reshape(H, W, 4).copy()
        assert np.array_equal(m[..., 0], lum(img[..., :3])) or frames > 1   # one frame: mean l is lum of the image
        m[..., 3] = frames                                                    # counted: what resolve() makes of it
        v = variance(m, gn, gp, p, np.float64)
        assert np.isfinite(v).all() and (v >= 0).all()
        out, vout = svgf_atrous(img, v.astype(np.float32), gn, gp, p, np.float64)
        old = atrous(img, gn, gp, mrt_mod.DenoiseParams.default(frames), np.float64)
        before, after, after_old = rel_mse(img, ref), rel_mse(out, ref), rel_mse(old, ref)
        print(f"{scene} {W}x{H} L={L} frames {frames}: relMSE {before:.5f} -> variance-guided {after:.5f} "
              f"(ratio {after / before:.3f}), existing filter {after_old:.5f} (ratio {after_old / before:.3f})")
        assert np.isfinite(out).all() and np.isfinite(vout).all()
        assert after < before
