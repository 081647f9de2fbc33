"""Host side of adaptive sampling (include/mrt.h "adaptive sampling", DESIGN.md
§2.1q): the parameters and their check (libmrt, no device), the numpy models
of merge, priority and selection (tests/adaptive_model.py) on hand-built cases, and the equal-budget quality
study of the definitions on oracle renders."""
import numpy as np
import pytest

from adaptive_model import accumulate64, counted_merge, tile_mask, tile_pixels, tile_priority, tile_select, tiles_of
from denoise_model import rel_mse
from helpers import SEED, host_threads
from test_denoise_host import oracle_guides
from variance_model import lum, variance

MISS = np.uint32(0xFFFFFFFF).view(np.float32)


# ---- parameters ------------------------------------------------------
def test_default_params(mrt_mod):
    p = mrt_mod.AdaptiveParams.default()
    assert p.luminance_floor == np.float32(0.01)
    p.check()
    assert p.as_dict() == {"luminance_floor": p.luminance_floor}


@pytest.mark.parametrize("value", [0.0, -0.01, float("nan"), float("inf")])
def test_check_rejects_bad_floor(mrt_mod, value):
    with pytest.raises(mrt_mod.MrtError, match="luminance_floor") as e:
        mrt_mod.AdaptiveParams(value).check()
    assert e.value.status == -1   # MRT_ERR_INVALID
    mrt_mod.AdaptiveParams(1e-30).check()
    assert mrt_mod.lib().mrt_adaptive_params_check(None) == -1
    assert mrt_mod.lib().mrt_adaptive_params_default(None) == -1


# ---- the models on hand-built cases ---------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_merge_model(dtype):
    a = np.array([[1.0, 2.0, 3.0, 2.0], [1.0, 2.0, 3.0, 0.0], [np.nan, 2.0, 3.0, 2.0], [1.0, 2.0, 3.0, 2.0],
                  [0.5, 0.5, 0.5, 0.0], [1.0, 2.0, 3.0, 1.0]], np.float32)
    b = np.array([[3.0, 4.0, 5.0, 6.0], [3.0, 4.0, 5.0, 6.0], [3.0, 4.0, 5.0, 6.0], [3.0, np.inf, 5.0, 6.0],
                  [9.0, 9.0, np.nan, 0.0], [4.0, 4.0, 4.0, 3.0]], np.float32)
    out = counted_merge(a, b, dtype)
    assert out.dtype == dtype
    assert (out[0] == [2.5, 3.5, 4.5, 8.0]).all()                      # (2 a + 6 b) / 8
    assert out[1].astype(np.float32).tobytes() == b[1].tobytes()       # ha == 0: b
    assert out[2].astype(np.float32).tobytes() == b[2].tobytes()       # a not finite: b
    assert out[3].astype(np.float32).tobytes() == a[3].tobytes()       # b not finite: a
    assert out[4].astype(np.float32).tobytes() == a[4].tobytes()       # hb == 0: a, empty or not
    assert (out[5] == [3.25, 3.5, 3.75, 4.0]).all()
    assert counted_merge(a.reshape(2, 3, 4), b.reshape(2, 3, 4), dtype).shape == (2, 3, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_priority_model(dtype):
    W, H = 130, 70                                                     # 3 x 2 tiles, the last column 2 px, the top row 6 px
    img = np.zeros((H, W, 4), np.float32)
    img[..., :3] = 0.5
    var = np.full((H, W), 0.25, np.float32)
    gn = np.zeros((H, W, 4), np.float32)
    gn[:64, 64:128, 3] = MISS                                          # tile 1: no filterable pixel
    gn[0, 0, 3] = np.uint32(0x80000003).view(np.float32)               # a light pixel in tile 0
    img[1, 1, 2] = np.inf                                              # a non-finite pixel in tile 0
    img[2, 2, 3] = np.nan                                              # (the count channel does not matter)
    eps = np.float32(0.01)
    p = tile_priority(img, var, gn, eps, dtype)
    assert p.shape == (6,) and p.dtype == dtype
    l = float(lum(np.float32([0.5, 0.5, 0.5]), np.float64))
    term = 0.25 / (l * l + float(eps) * float(eps))
    pixels = np.array([64 * 64 - 2, 0, 2 * 64, 64 * 6, 64 * 6, 2 * 6], np.float64)
    np.testing.assert_allclose(p.astype(np.float64), term * pixels, rtol=1e-5 if dtype == np.float32 else 1e-7)
    assert p[1] == 0
    assert [tile_pixels(W, H, t) for t in range(6)] == [4096, 4096, 128, 384, 384, 12]
    # a dark, noisy tile outranks a bright one with the same variance: the measure is relative
    img[:64, :64, :3] = 0.05
    assert tile_priority(img, var, gn, eps, dtype)[0] > 50 * p[0]


def test_select_model():
    assert (tile_select(np.full(9, 0.5, np.float32), 4) == [0, 1, 2, 3]).all()            # all equal: 0..K-1
    assert (tile_select(np.zeros(5, np.float32), 5) == np.arange(5)).all()
    pri = np.array([1.0, -3.0, np.nan, 2.0, np.inf, 0.0, -np.inf, 2.0], np.float32)
    assert (tile_select(pri, 8) == [3, 7, 0, 1, 2, 4, 5, 6]).all()       # negative and non-finite count as 0; K = T
    assert (tile_select(pri, 1) == [3]).all() and tile_select(pri, 3).dtype == np.uint32
    rng = np.random.default_rng(5)
    p = rng.uniform(0, 1, 1000).astype(np.float32)
    got = tile_select(p, 1000)
    assert sorted(got.tolist()) == list(range(1000)) and (np.diff(p[got]) <= 0).all()


def test_tile_mask():
    m = tile_mask(160, 96, [5, 0])
    assert m.sum() == 64 * 64 + 32 * 32 and m[0, 0] == 1 and m[95, 159] == 1 and m[0, 64] == 0 and m[64, 0] == 0
    assert tiles_of(160, 96) == (3, 2) and tiles_of(64, 64) == (1, 1) and tiles_of(65, 1) == (2, 1)


# ---- equal-budget quality study -----------------------------------------------------
STUDY_W, STUDY_H, STUDY_L, STUDY_B = 192, 128, 4, 16
STUDY_CONFIGS = [(4, 4, 3), (4, 6, 2)]   # (passes, frames, tiles): 48 tile-frames each
# where the measured gain over uniform exceeded the seed-to-seed spread of the uniform renders (the docstring
# of test_equal_budget_study): only there is "adaptive <= uniform" asserted
STUDY_WINS = {("cornellbox", (4, 4, 3)), ("cornellbox", (4, 6, 2))}
STUDY_SEEDS = (SEED, SEED + 101, SEED + 202)


def adaptive_render(oracle_mod, mrt_mod, osc, guides, seed, base_frames, passes, frames, K):
    """The renderer's refine loop in float64 through the models: base_frames uniform frames, then `passes`
    passes of `frames` extra frames of the K tiles of highest priority.  Returns (image, samples per pixel,
    tile-frames spent by the passes)."""
    W, H, L = STUDY_W, STUDY_H, STUDY_L
    gn, gp = guides
    sp, ap = mrt_mod.SvgfParams.default(), mrt_mod.AdaptiveParams.default()
    one = lambda s, f, mask=None: osc.render(W, H, L, s, 1, frame_begin=f, threads=host_threads(), pixel_mask=mask,   # noqa: E731
                                            flags=oracle_mod.NO_ACCUMULATE)[0][..., :3].astype(np.float64)
    c = np.zeros((H, W, 3))
    m = np.zeros((H, W, 2))
    n = np.zeros((H, W))
    def add(rgb, mask):
        nonlocal c, m
        l = lum(rgb.astype(np.float32), np.float64)
        sel = mask.astype(bool)
        c[sel] = accumulate64(c, rgb, n)[sel]
        m[sel] = accumulate64(m, np.stack([l, l * l], -1), n)[sel]
        n[sel] += 1
    full = np.ones((H, W), np.uint8)
    for f in range(base_frames):
        add(one(seed, f), full)
    e = spent = 0
    for _ in range(passes):
        mom = np.concatenate([m, np.zeros((H, W, 1)), n[..., None]], -1).astype(np.float32)
        img = np.concatenate([c, n[..., None]], -1).astype(np.float32)
        v = variance(mom, gn, gp, sp, np.float64)
        lst = tile_select(tile_priority(img, v, gn, ap.luminance_floor, np.float64), K)
        mask = tile_mask(W, H, lst)
        for _ in range(frames):
            add(one(seed ^ mrt_mod.REFINE_SEED_XOR, e, mask), mask)
            e += 1
        spent += K * frames
    return np.concatenate([c, n[..., None]], -1), n, spent


@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_equal_budget_study(mrt_mod, oracle_mod, scene):
    """Uniform B = 16 frames against 8 uniform frames plus refine passes that spend the other 8 x 6 tile-frames,
    at 192x128 (6 tiles), L = 4; relMSE against an independently seeded 256-frame oracle render, three seeds.

    Measured with this test (mean relMSE over the seeds, (passes, frames, tiles)):
      cornellbox        uniform 0.00633, spread over the seeds 0.00029, 8 frames alone 0.01212;
                        (4, 4, 3) 0.00555, (8, 2, 3) 0.00553, (4, 6, 2) 0.00525, (8, 1, 6) 0.00641
      CornellBox-Water  uniform 0.04155, spread 0.00622, 8 frames alone 0.08010;
                        (4, 4, 3) 0.03943, (8, 2, 3) 0.03975, (4, 6, 2) 0.03954, (8, 1, 6) 0.04175
    ((8, 2, 3) and the control (8, 1, 6) — every tile every pass, which is uniform sampling with the refine
    seed — were measured once and are not run here, to keep the test short.)  On cornellbox the gain of the
    configurations that choose (0.0008 to 0.0011) is 2.7 to 3.7 times the spread: asserted.  On
    CornellBox-Water the gain (0.002) is a third of the spread: adaptive is ahead in the mean, which these
    three seeds cannot tell from chance, so nothing about its quality is asserted.  Everywhere: the budget
    accounting exactly, and that adaptive stays below the 8 base frames alone."""
    W, H, L, B = STUDY_W, STUDY_H, STUDY_L, STUDY_B
    T = tiles_of(W, H)[0] * tiles_of(W, H)[1]
    assert T == 6
    osc = oracle_mod.OracleScene(mrt_mod.scene_path(scene))
    guides = oracle_guides(oracle_mod, osc, W, H)
    ref, _ = osc.render(W, H, L, SEED + 7, 256, threads=host_threads())
    uniform, base, adaptive = [], [], {cfg: [] for cfg in STUDY_CONFIGS}
    for seed in STUDY_SEEDS:
        uniform.append(rel_mse(osc.render(W, H, L, seed, B, threads=host_threads())[0], ref))
        base.append(rel_mse(osc.render(W, H, L, seed, B // 2, threads=host_threads())[0], ref))
        for cfg in STUDY_CONFIGS:
            img, n, spent = adaptive_render(oracle_mod, mrt_mod, osc, guides, seed, B // 2, *cfg)
            # the budget, exactly: the same number of tile-frames as the uniform render, pixel by pixel accounted
            assert spent == (B // 2) * T and (B // 2) * T + spent == B * T
            assert n.min() >= B // 2 and float(n.sum()) <= B * W * H
            per_tile = [n[tile_mask(W, H, [t]).astype(bool)] for t in range(T)]
            assert all((p == p.flat[0]).all() for p in per_tile)                       # whole tiles only
            assert sum(int(p.flat[0]) - B // 2 for p in per_tile) == spent
            adaptive[cfg].append(rel_mse(img.astype(np.float32), ref))
    u, spread = float(np.mean(uniform)), float(np.max(uniform) - np.min(uniform))
    print(f"{scene} {W}x{H} L={L}: uniform {B} frames relMSE {u:.5f} (seeds {['%.5f' % x for x in uniform]}, "
          f"spread {spread:.5f}); {B // 2} frames alone {np.mean(base):.5f}")
    for cfg, vals in adaptive.items():
        a = float(np.mean(vals))
        print(f"  adaptive passes x frames x tiles {cfg}: relMSE {a:.5f} ({['%.5f' % x for x in vals]}), "
              f"ratio to uniform {a / u:.3f}, gap {u - a:+.5f} against spread {spread:.5f}")
        assert a < float(np.mean(base))
        if (scene, cfg) in STUDY_WINS:
            assert a <= u
