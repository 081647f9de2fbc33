"""Host side of the denoiser: the default parameters and their check (libmrt,
no device), and the quality gate of the filter's definition — the numpy model
(tests/denoise_model.py) on oracle renders, with guide planes built from the
oracle's own camera rays and nearest hits."""
import math

import numpy as np
import pytest

from denoise_model import NOT_FILTERABLE, atrous, guides_from_hits, rel_mse, words
from helpers import SEED, host_threads


@pytest.mark.parametrize("frames,iterations", [(0, 3), (1, 3), (2, 3), (3, 2), (16, 2), (17, 1), (10 ** 6, 1)])
def test_default_params(mrt_mod, frames, iterations):
    p = mrt_mod.DenoiseParams.default(frames)
    assert p.iterations == iterations
    assert p.sigma_color == np.float32(2.0 / math.sqrt(max(frames, 1)))
    assert p.sigma_plane == np.float32(0.01)
    assert p.normal_log2_power == 6
    p.check()


@pytest.mark.parametrize("field,value", [
    ("iterations", 9), ("normal_log2_power", 9),
    ("sigma_color", -1.0), ("sigma_color", float("nan")), ("sigma_color", float("inf")),
    ("sigma_plane", 0.0), ("sigma_plane", -0.01), ("sigma_plane", float("nan")), ("sigma_plane", float("inf")),
])
def test_check_rejects_bad_fields(mrt_mod, field, value):
    p = mrt_mod.DenoiseParams.default(4)
    setattr(p, field, value)
    with pytest.raises(mrt_mod.MrtError, match=field) as e:
        p.check()
    assert e.value.status == -1   # MRT_ERR_INVALID
    # the extremes of each range pass
    q = mrt_mod.DenoiseParams(8, 0.0, 1e-6, 8)
    q.check()
    mrt_mod.DenoiseParams(0, 3.0, 10.0, 0).check()


def test_null_params_rejected(mrt_mod):
    assert mrt_mod.lib().mrt_denoise_params_check(None) == -1
    assert mrt_mod.lib().mrt_denoise_params_default(1, None) == -1


def oracle_guides(oracle_mod, osc, W, H):
    """The guide planes of the reference's camera from the oracle's stages:
    raygen with a constant-0.5 noise table (the pixel-centre ray) + brute-force
    nearest hits + the scene arrays."""
    rays = oracle_mod.raygen(W, H, np.full(64 * 64 * 4, 0.5, np.float32))
    gn, gp = guides_from_hits(osc, osc.intersect(rays), rays)
    return gn.reshape(H, W, 4), gp.reshape(H, W, 4)


@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_model_quality_gate(mrt_mod, oracle_mod, scene):
    """Denoised relMSE < undenoised relMSE against an independently seeded
    256-frame reference, for 1, 4 and 16 accumulated frames with the library's
    default parameters.  Ratios denoised / undenoised measured with this test
    (96x64, L = 4): cornellbox 0.112 / 0.193 / 0.406, CornellBox-Water
    0.540 / 0.467 / 0.398 (DESIGN.md "Denoised output")."""
    W, H, L = 96, 64, 4
    osc = oracle_mod.OracleScene(mrt_mod.scene_path(scene))
    gn, gp = oracle_guides(oracle_mod, osc, W, H)
    w = words(gn)
    assert (w < NOT_FILTERABLE).mean() > 0.5 and (w >= NOT_FILTERABLE).any()
    ref, _ = osc.render(W, H, L, SEED + 1, 256, frame_begin=0, threads=host_threads())
    for frames in (1, 4, 16):
        img, _ = osc.render(W, H, L, SEED, frames, threads=host_threads())
        out = atrous(img, gn, gp, mrt_mod.DenoiseParams.default(frames), np.float64)
        before, after = rel_mse(img, ref), rel_mse(out, ref)
        print(f"{scene} {W}x{H} L={L} frames {frames}: relMSE {before:.5f} -> {after:.5f}, ratio {after / before:.3f}")
        assert np.isfinite(out).all()
        assert after < before
