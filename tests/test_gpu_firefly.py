"""Firefly suppression on the device: the stage call mrt_firefly_clamp against
the float64 model of its definition (tests/firefly_model.py) on the synthetic
inputs of test_gpu_denoise.py with planted fireflies, its argument errors, the
renderer layer (set_firefly, read_clamped, denoise_variance, error_estimate,
converge, the CLI's --firefly) against a replay through the stage calls, and
the quality on CornellBox-Water.

Tolerance of the model comparison: four times the largest deviation of the
float32 model from the float64 model on the same inputs (test_firefly_host.py
model_pair), printed per case.  A pixel whose l_p and cap agree within that
tolerance in the float64 model is undecided and left out; the host test bounds
their share."""
import os
import subprocess

import numpy as np
import pytest

from denoise_model import NOT_FILTERABLE, rel_mse, words
from helpers import SEED, dev_ptr, from_dev, host_threads, to_dev
from test_firefly_host import SIZES, model_pair

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5


def status_of(mrt_mod, fn, *args, **kw):
    with pytest.raises(mrt_mod.MrtError) as e:
        fn(*args, **kw)
    return e.value.status


def gpu_clamp(mrt_mod, img, gn, gp, params, count=True):
    """(out [H, W, 4], clamped) of mrt_firefly_clamp on device copies; the inputs are only read."""
    H, W = img.shape[:2]
    bufs = [to_dev(np.ascontiguousarray(v, np.float32)) for v in (img, gn, gp)]
    d_out = to_dev(np.full((H, W, 4), -7.0, np.float32))
    d_cnt = to_dev(np.array([0xDEADBEEF], np.uint32))
    mrt_mod.firefly_clamp(dev_ptr(bufs[0]), dev_ptr(bufs[1]), dev_ptr(bufs[2]), dev_ptr(d_out),
                          dev_ptr(d_cnt) if count else None, W, H, params)
    for b, v in zip(bufs, (img, gn, gp)):
        assert from_dev(b, np.float32).tobytes() == np.ascontiguousarray(v).tobytes()
    return from_dev(d_out, np.float32).reshape(H, W, 4), int(from_dev(d_cnt, np.uint32)[0])


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("W,H", SIZES)
def test_clamp_matches_model(gpu, mrt_mod, W, H, R):
    (img, gn, gp), m64, m32, tol, und = model_pair(W, H, R)
    p = mrt_mod.FireflyParams.default()
    p.radius = R
    got, count = gpu_clamp(mrt_mod, img, gn, gp, p)
    out64, _, mask64, _ = m64
    changed = (got[..., :3].view(np.uint32) != img[..., :3].view(np.uint32)).any(-1)
    filt = words(gn) < NOT_FILTERABLE
    ok = ~und
    err = float(np.abs(got[mask64 & ok].astype(np.float64) - out64[mask64 & ok]).max()) if (mask64 & ok).any() else 0.0
    print(f"{W}x{H} R={R}: tolerance {tol:.3g}, kernel error {err:.3g}, clamped {count} (model {int(mask64.sum())}), "
          f"undecided {int(und.sum())}")
    assert np.array_equal(changed[ok], mask64[ok])                           # the decision is the model's
    assert got[~changed].tobytes() == img[~changed].tobytes()                # unclamped: bitwise, alpha included
    assert got[~filt].tobytes() == img[~filt].tobytes()                      # misses and lights
    assert got[..., 3].tobytes() == img[..., 3].tobytes()                    # alpha
    assert np.isfinite(got[mask64 & ok]).all() and err <= tol
    assert count == int(changed.sum())
    if W >= 16 and H >= 8:
        assert count >= 3
    # the count is optional, and the image does not depend on it
    alone, untouched = gpu_clamp(mrt_mod, img, gn, gp, p, count=False)
    assert alone.tobytes() == got.tobytes() and untouched == 0xDEADBEEF


def test_argument_errors_leave_out_untouched(gpu, mrt_mod):
    W, H = 53, 37
    n = W * H * 4
    d = [to_dev(np.zeros(n, np.float32)) for _ in range(3)]
    d_out = to_dev(np.full(n + 4, -7.0, np.float32))
    d_cnt = to_dev(np.array([77, 0, 0, 0], np.uint32))
    i, g1, g2 = (dev_ptr(t) for t in d)
    o, c = dev_ptr(d_out), dev_ptr(d_cnt)
    p = mrt_mod.FireflyParams.default()
    for args in [(i, g1, g2, i, c), (i, g1, g2, i + 16, c), (i, g1, g2, g1, c), (i, g1, g2, g2 + 64, c),
                 (i, g1, g2, o, i), (i, g1, g2, o, g1 + 4), (i, g1, g2, o, g2 + 4 * n - 4), (i, g1, g2, o, o),
                 (i, g1, g2, o, o + 4 * n - 4), (0, g1, g2, o, c), (i, 0, g2, o, c), (i, g1, 0, o, c),
                 (i, g1, g2, 0, c)]:
        assert status_of(mrt_mod, mrt_mod.firefly_clamp, *args, W, H, p) == ERR_INVALID, args
    assert status_of(mrt_mod, mrt_mod.firefly_clamp, i, g1, g2, o, c, W, H, None) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.firefly_clamp, i, g1, g2, o, c, 0, H, p) == ERR_INVALID
    for field, value in (("radius", 0), ("radius", 4), ("k", 0.0), ("k", float("nan")), ("min_taps", 0),
                         ("normal_cos_min", 2.0), ("plane_tolerance", -1.0)):
        bad = mrt_mod.FireflyParams.default()
        setattr(bad, field, value)
        with pytest.raises(mrt_mod.MrtError, match=field):
            mrt_mod.firefly_clamp(i, g1, g2, o, c, W, H, bad)
    assert (from_dev(d_out, np.float32) == -7.0).all() and from_dev(d_cnt, np.uint32)[0] == 77
    mrt_mod.firefly_clamp(i, g1, g2, o, o + 4 * n, W, H, p)                  # the counter right behind `out` is fine
    assert (from_dev(d_out, np.float32)[:n] == 0.0).all() and from_dev(d_out, np.uint32)[n] == 0


# ---- renderer layer ----------------------------------------------------------
W0, H0, L0 = 64, 48, 4


def _scene(mrt_mod, name, cache={}):
    if name not in cache:
        cache[name] = mrt_mod.Scene(name)
    return cache[name]


def replay(mrt_mod, sc, r, precise, fp, sp=None):
    """(clamped, count, variance, denoised) of the stage calls on what the
    renderer holds: read_resolved -> firefly_clamp (fp None: none) -> variance
    of the resolved moments -> denoise_variance."""
    H, W = r.height, r.width
    frames = r.stats()["frame_index"]
    sp = sp or mrt_mod.SvgfParams.default()
    buf = lambda c=4: to_dev(np.zeros((H, W, c), np.float32))   # noqa: E731
    d_n, d_p, d_res, d_cl, d_mres, d_out, d_scr, d_var = buf(), buf(), to_dev(r.read_resolved()), buf(), buf(), buf(), \
        buf(), buf(1)
    d_cnt = to_dev(np.array([0xDEADBEEF], np.uint32))
    d_mom = to_dev(r.read_moments())
    mrt_mod.guides(sc, W, H, dev_ptr(d_n), dev_ptr(d_p), camera=r.camera, precise=precise)
    mrt_mod.temporal_resolve(dev_ptr(d_mom), frames, None, dev_ptr(d_mres), W, H)
    src = d_res
    if fp is not None:
        mrt_mod.firefly_clamp(dev_ptr(d_res), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_cl), dev_ptr(d_cnt), W, H, fp)
        src = d_cl
    mrt_mod.variance(dev_ptr(d_mres), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_var), W, H, sp)
    mrt_mod.denoise_variance(dev_ptr(src), dev_ptr(d_var), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_out), dev_ptr(d_scr),
                             None, W, H, sp)
    host = lambda t, c=4: from_dev(t, np.float32).reshape(H, W, c)   # noqa: E731
    return host(d_cl), int(from_dev(d_cnt, np.uint32)[0]), host(d_var, 1)[..., 0], host(d_out)


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("scene", ["cornellbox", "CornellBox-Water"])
def test_renderer_firefly_equals_stage_replay(gpu, mrt_mod, scene, precise):
    sc = _scene(mrt_mod, scene)
    fp = mrt_mod.FireflyParams.default()
    never = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise, moments=True)
    never.draw(4)
    never.denoise_variance()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise, moments=True)
    assert r.firefly is None
    assert status_of(mrt_mod, r.read_clamped) == ERR_STATE
    with pytest.raises(mrt_mod.MrtError, match="radius"):                 # a failed check changes nothing
        r.set_firefly(mrt_mod.FireflyParams(4, 3.0, 3, 0.9, 0.01))
    assert r.firefly is None
    r.set_firefly(fp)
    assert r.firefly.as_dict() == fp.as_dict()
    r.draw(4)
    r.denoise_variance()             # enqueued behind the draw, no sync in between
    den, (cl, count) = r.read_denoised(), r.read_clamped()
    want_cl, want_count, want_var, want = replay(mrt_mod, sc, r, precise, fp)
    assert cl.tobytes() == want_cl.tobytes() and count == want_count
    assert den.tobytes() == want.tobytes() and r.read_variance().tobytes() == want_var.tobytes()
    res = r.read_resolved()
    changed = (cl.view(np.uint32) != res.view(np.uint32)).any(-1)
    print(f"{scene} precise={precise}: clamped {count} of {W0 * H0} pixels")
    assert count == int(changed.sum()) and 0 < count < W0 * H0 // 4
    # nothing else is written: image, moments, resolved and variance are a never-set renderer's
    assert r.read_image().tobytes() == never.read_image().tobytes()
    assert r.read_moments().tobytes() == never.read_moments().tobytes()
    assert res.tobytes() == never.read_resolved().tobytes()
    assert r.read_variance().tobytes() == never.read_variance().tobytes()
    assert den.tobytes() != never.read_denoised().tobytes()
    # the estimate and the stop rule run on the clamped pipeline
    s = r.error_estimate(0.0)
    assert np.isfinite(s["frame_error"]) and np.isfinite(s["max_tile_error"]) and s["pixels"] > 0
    assert r.read_denoised().tobytes() == den.tobytes() and r.read_clamped()[0].tobytes() == cl.tobytes()
    res_c = r.converge(target_error=0.5 * s["max_tile_error"], frames_per_pass=2, max_passes=2)
    assert np.isfinite(res_c["last"]["frame_error"]) and res_c["passes"] >= 1
    _, _, _, want = replay_resolved(mrt_mod, sc, r, precise, fp)
    assert r.read_denoised().tobytes() == want.tobytes()                  # the denoised buffer is current
    assert r.read_image().tobytes() == never.read_image().tobytes()
    # explicit parameters
    q = mrt_mod.FireflyParams(1, 1.5, 2, 0.8, 0.02)
    r.set_firefly(q)
    r.denoise_variance()
    want_cl, want_count, _, want = replay_resolved(mrt_mod, sc, r, precise, q)
    assert r.read_clamped()[0].tobytes() == want_cl.tobytes() and r.read_clamped()[1] == want_count
    assert r.read_denoised().tobytes() == want.tobytes()
    r.close()
    # off again: the never-set renderer's result, bitwise
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=precise, moments=True)
    r.set_firefly(fp)
    r.draw(4)
    r.denoise_variance()
    r.set_firefly(None)
    assert r.firefly is None
    r.denoise_variance()
    assert r.read_denoised().tobytes() == never.read_denoised().tobytes()
    assert r.read_clamped()[0].tobytes() == cl.tobytes()                  # the last clamp's buffer stays readable
    # the setting survives reset, a move and a resize
    r.set_firefly(fp)
    r.reset()
    assert r.firefly.as_dict() == fp.as_dict()
    r.draw(2)
    cam = mrt_mod.Camera.look_at((0.1, 1.0, 2.35), (0.0, 1.0, 1.35), (0.0, 1.0, 0.0), 90.0)
    r.move_camera(cam)
    assert r.firefly.as_dict() == fp.as_dict()
    r.draw(2)
    r.denoise_variance()
    want_cl, want_count, _, want = replay_resolved(mrt_mod, sc, r, precise, fp)
    assert r.read_clamped()[0].tobytes() == want_cl.tobytes() and r.read_clamped()[1] == want_count
    assert r.read_denoised().tobytes() == want.tobytes()
    r.resize(48, 40)
    assert r.firefly.as_dict() == fp.as_dict()
    assert status_of(mrt_mod, r.read_clamped) == ERR_STATE
    r.draw(2)
    r.denoise_variance()
    want_cl, want_count, _, want = replay_resolved(mrt_mod, sc, r, precise, fp)
    assert r.read_clamped()[0].shape == (40, 48, 4) and r.read_clamped()[0].tobytes() == want_cl.tobytes()
    assert r.read_clamped()[1] == want_count and r.read_denoised().tobytes() == want.tobytes()
    r.close()
    never.close()


def replay_resolved(mrt_mod, sc, r, precise, fp):
    """As replay, from the renderer's own resolved buffer and variance plane (a
    renderer with extra samples or a history resolves more than its image)."""
    H, W = r.height, r.width
    sp = mrt_mod.SvgfParams.default()
    buf = lambda c=4: to_dev(np.zeros((H, W, c), np.float32))   # noqa: E731
    d_n, d_p, d_cl, d_out, d_scr = buf(), buf(), buf(), buf(), buf()
    d_res, d_var = to_dev(r.read_resolved()), to_dev(r.read_variance())
    d_cnt = to_dev(np.array([0xDEADBEEF], np.uint32))
    mrt_mod.guides(sc, W, H, dev_ptr(d_n), dev_ptr(d_p), camera=r.camera, precise=precise)
    mrt_mod.firefly_clamp(dev_ptr(d_res), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_cl), dev_ptr(d_cnt), W, H, fp)
    mrt_mod.denoise_variance(dev_ptr(d_cl), dev_ptr(d_var), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_out), dev_ptr(d_scr),
                             None, W, H, sp)
    host = lambda t: from_dev(t, np.float32).reshape(H, W, 4)   # noqa: E731
    return host(d_cl), int(from_dev(d_cnt, np.uint32)[0]), None, host(d_out)


def test_needs_moments(gpu, mrt_mod):
    r = mrt_mod.Renderer(_scene(mrt_mod, "cornellbox"), W0, H0, L0)
    assert status_of(mrt_mod, r.set_firefly, mrt_mod.FireflyParams.default()) == ERR_STATE
    assert status_of(mrt_mod, r.set_firefly, None) == ERR_STATE
    assert r.firefly is None
    assert status_of(mrt_mod, r.read_clamped) == ERR_STATE
    r.close()


def test_quality_on_water(gpu, mrt_mod, oracle_mod):
    """CornellBox-Water 96x64, one frame, fast build: relMSE of the denoised image against a 256-frame oracle
    reference of another seed is lower with the clamp than without."""
    W, H, L = 96, 64, 4
    osc = oracle_mod.OracleScene(mrt_mod.scene_path("CornellBox-Water"))
    ref, _ = osc.render(W, H, L, SEED + 1, 256, frame_begin=0, threads=host_threads())
    r = mrt_mod.Renderer(_scene(mrt_mod, "CornellBox-Water"), W, H, L, precise=False, moments=True)
    r.draw(1)
    r.denoise_variance()
    without = rel_mse(r.read_denoised(), ref)
    r.set_firefly(mrt_mod.FireflyParams.default())
    r.denoise_variance()
    with_clamp = rel_mse(r.read_denoised(), ref)
    count = r.read_clamped()[1]
    undenoised = rel_mse(r.read_image(), ref)
    r.close()
    print(f"CornellBox-Water {W}x{H} 1 frame: relMSE undenoised {undenoised:.5f}, filter alone {without:.5f}, "
          f"clamp + filter {with_clamp:.5f} (ratio {with_clamp / without:.3f}), {count} pixels clamped")
    assert with_clamp < without


def test_cli_firefly(gpu, mrt_mod, tmp_path):
    """mrt_render --firefly writes the clamped pipeline's denoised image; the flag needs a variance-guided mode."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    base = [exe, "--scene", "CornellBox-Water", "--w", "64", "--h", "48", "--spp", "2", "--L", "4", "--precise"]

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
    r = mrt_mod.Renderer(_scene(mrt_mod, "CornellBox-Water"), 64, 48, 4, precise=True, moments=True)
    r.draw(2)
    r.denoise_variance()
    plain = r.read_denoised()
    r.set_firefly(mrt_mod.FireflyParams.default())
    r.denoise_variance()
    want = r.read_denoised()
    got = run(["--denoise-variance", "--firefly"], "a.pfm")
    assert got.tobytes() == rgb(want) and got.tobytes() != rgb(plain)
    assert run(["--firefly", "--denoise-variance"], "b.pfm").tobytes() == rgb(want)   # the value is optional
    p = mrt_mod.FireflyParams.default()
    p.k = 1.5
    r.set_firefly(p)
    r.denoise_variance()
    got = run(["--denoise-variance", "--firefly", "1.5"], "c.pfm")
    assert got.tobytes() == rgb(r.read_denoised()) and got.tobytes() != rgb(want)
    r.close()
    for extra in ([], ["--denoise"]):
        q = subprocess.run(base + ["--firefly"] + extra, capture_output=True, text=True, timeout=60)
        assert q.returncode != 0 and "--firefly needs" in q.stderr and "usage" in q.stderr
    q = subprocess.run(base + ["--denoise-variance", "--firefly", "-1"], capture_output=True, text=True, timeout=60)
    assert q.returncode != 0 and "k must be" in q.stderr
