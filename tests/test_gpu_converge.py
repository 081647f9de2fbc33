"""Sampling to a target error on the device (include/mrt.h "adaptive sampling",
DESIGN.md §2.1r): the stage calls mrt_tile_error and mrt_tile_threshold against
tests/converge_model.py, the renderer layer (error_estimate, converge, the
reader, the CLI) against the stage pipeline, and the stop rule.

Tolerances: the counts, the list and the integers of the summary are exact.
The means of mrt_tile_error and the summary's frame_error (their summation
order is free) are held to the rule of test_gpu_adaptive.within: four times the
largest deviation of the float32 model from the float64 model on the same
inputs, computed and printed per case.  max_tile_error is one of the inputs:
exact."""
import json
import os
import subprocess

import numpy as np
import pytest

from adaptive_model import tile_mask, tiles_of
from converge_model import tile_error, tile_threshold
from helpers import dev_ptr, from_dev, to_dev
from test_gpu_adaptive import ERR_INVALID, ERR_STATE, L0, H0, W0, Stage, _scene, rendered_planes, status_of, within

pytestmark = pytest.mark.gpu

MISS = np.uint32(0xFFFFFFFF).view(np.float32)


# ---- mrt_tile_error ------------------------------------------------------------------
def error_inputs(mrt_mod, W, H):
    """rendered_planes with pixels that do not count: a non-finite one, and at 160x96 a tile without any and
    part of another unfilterable."""
    if (W, H) == (1, 1):                                               # one pixel that counts, of the 64x64 render
        img, var, gn = rendered_planes(mrt_mod, 64, 64)
        ok = (gn[..., 3].view(np.uint32) < 0x80000000) & (var > 0) & (img[..., :3].max(-1) > 0)
        y, x = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
        return tuple(np.ascontiguousarray(v[y:y + 1, x:x + 1]) for v in (img, var, gn))
    img, var, gn = (v.copy() for v in rendered_planes(mrt_mod, W, H))
    if W * H > 200:
        img[H // 2, W // 3, 1] = np.nan
        img[H // 3, W // 2, 0] = np.inf
    if (W, H) == (160, 96):
        gn[:64, 64:128, 3] = MISS                                      # tile 1: no counted pixel
        gn[70:80, 5:50, 3] = np.uint32(0x80000001).view(np.float32)    # unfilterable pixels in tile 3
    return img, var, gn


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("W,H", [(160, 96), (65, 1), (64, 64), (1, 1)])
def test_tile_error(gpu, mrt_mod, W, H, precise):
    img, var, gn = error_inputs(mrt_mod, W, H)
    p = mrt_mod.AdaptiveParams.default()
    tx, ty = tiles_of(W, H)
    d = [to_dev(v) for v in (img, var, gn)]
    d_e, d_n = to_dev(np.full(tx * ty, -3.0, np.float32)), to_dev(np.full(tx * ty, 77, np.uint32))
    mrt_mod.tile_error(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_e), dev_ptr(d_n), W, H, p, precise=precise)
    got, got_n = from_dev(d_e, np.float32), from_dev(d_n, np.uint32)
    m64, n64 = tile_error(img, var, gn, p.luminance_floor, np.float64)
    m32, _ = tile_error(img, var, gn, p.luminance_floor, np.float32)
    assert (got_n == n64).all()                                        # the counts: exact
    assert np.isfinite(m64).all() and (got >= 0).all() and m64.max() > 0
    scale = np.maximum(m64, 1e-30)                                     # relative to each tile's own mean
    within(f"mrt_tile_error {W}x{H} {'precise' if precise else 'fast'}", got / scale, m64 / scale,
           m32.astype(np.float64) / scale)
    assert (got[n64 == 0] == 0).all()
    if (W, H) == (160, 96):
        assert n64[1] == 0 and n64[3] <= 64 * 32 - 10 * 45 and (n64[[0, 2, 3, 4, 5]] > 0).all()
    for k, t in enumerate(d):
        assert from_dev(t, np.float32).tobytes() == (img, var, gn)[k].tobytes()


def test_tile_error_argument_errors(gpu, mrt_mod):
    W, H = 160, 96
    img, var, gn = error_inputs(mrt_mod, W, H)
    p = mrt_mod.AdaptiveParams.default()
    d = [to_dev(v) for v in (img, var, gn)]
    d_e, d_n = to_dev(np.zeros(8, np.float32)), to_dev(np.zeros(8, np.uint32))
    call = lambda e, n, prm: mrt_mod.tile_error(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), e, n, W, H, prm)   # noqa: E731
    assert status_of(mrt_mod, call, dev_ptr(d_e), dev_ptr(d_n), None) == ERR_INVALID
    for t in d:                                                        # an output inside an input
        assert status_of(mrt_mod, call, dev_ptr(t) + 8, dev_ptr(d_n), p) == ERR_INVALID
        assert status_of(mrt_mod, call, dev_ptr(d_e), dev_ptr(t) + 8, p) == ERR_INVALID
    assert status_of(mrt_mod, call, dev_ptr(d_e), dev_ptr(d_e) + 8, p) == ERR_INVALID     # the outputs overlap
    with pytest.raises(mrt_mod.MrtError, match="luminance_floor"):
        call(dev_ptr(d_e), dev_ptr(d_n), mrt_mod.AdaptiveParams(0.0))
    assert not from_dev(d_e, np.float32).any() and not from_dev(d_n, np.uint32).any()


# ---- mrt_tile_threshold --------------------------------------------------------------
def gpu_threshold(mrt_mod, e, n, threshold, max_count):
    e, n = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(n, np.uint32)
    d_e, d_n = to_dev(e), to_dev(n)
    d_l, d_s = to_dev(np.full(max_count + 2, 0xFFFFFFFF, np.uint32)), to_dev(np.full(8, 0xFFFFFFFF, np.uint32))
    mrt_mod.tile_threshold(dev_ptr(d_e), dev_ptr(d_n), len(e), threshold, max_count, dev_ptr(d_l), dev_ptr(d_s))
    out = from_dev(d_l, np.uint32)
    s = mrt_mod.ErrorSummary.from_buffer_copy(from_dev(d_s, np.uint32).tobytes())
    assert s.reserved[0] == 0 and s.reserved[1] == 0
    assert from_dev(d_e, np.float32).tobytes() == e.tobytes() and (from_dev(d_n, np.uint32) == n).all()
    listed = s.tiles_listed
    assert (out[listed:] == 0xFFFFFFFF).all()                          # nothing behind the list is written
    return out[:listed], s.as_dict()


def check_threshold(mrt_mod, name, e, n, threshold, max_count):
    got, s = gpu_threshold(mrt_mod, e, n, threshold, max_count)
    want, m32 = tile_threshold(e, n, threshold, max_count, np.float32)
    _, m64 = tile_threshold(e, n, threshold, max_count, np.float64)
    assert (got == want).all() and len(got) == len(want)
    for k in ("tiles_above", "tiles_listed", "tiles_counted", "pixels"):
        assert s[k] == m32[k], k
    assert s["tiles_listed"] == min(s["tiles_above"], max_count)
    assert np.float32(s["max_tile_error"]) == m32["max_tile_error"]
    within(f"mrt_tile_threshold frame_error {name}", np.array([s["frame_error"]], np.float32),
           np.array([m64["frame_error"]], np.float64), np.array([m32["frame_error"]], np.float64))
    return got, s


def random_tiles(T, seed):
    rng = np.random.default_rng(seed)
    e = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), T)).astype(np.float32)
    n = rng.integers(1, 4097, T).astype(np.uint32)
    n[rng.choice(T, max(T // 50, 1), replace=False)] = 0               # tiles without a counted pixel
    return e, n


def test_tile_threshold_small(gpu, mrt_mod):
    got, s = check_threshold(mrt_mod, "T=1 above", [0.5], [7], 0.25, 1)
    assert got.tolist() == [0] and s["frame_error"] == 0.5
    got, s = check_threshold(mrt_mod, "T=1 at the threshold", [0.5], [7], 0.5, 1)
    assert got.tolist() == [] and s["tiles_above"] == 0
    # T = 7: ties, a key equal to the threshold, a negative, a NaN, a tile with pixels = 0
    e = np.array([2.0, 5.0, 2.0, -1.0, 5.0, np.nan, 9.0], np.float32)
    n = np.array([10, 20, 10, 10, 20, 10, 0], np.uint32)
    got, s = check_threshold(mrt_mod, "T=7 threshold 2", e, n, 2.0, 7)
    assert got.tolist() == [1, 4] and (s["tiles_counted"], s["pixels"], s["max_tile_error"]) == (6, 80, 5.0)
    got, s = check_threshold(mrt_mod, "T=7 threshold 1", e, n, 1.0, 7)
    assert got.tolist() == [1, 4, 0, 2]
    got, s = check_threshold(mrt_mod, "T=7 threshold 1, two listed", e, n, 1.0, 2)
    assert got.tolist() == [1, 4] and (s["tiles_above"], s["tiles_listed"]) == (4, 2)
    got, s = check_threshold(mrt_mod, "T=7 threshold 0", e, n, 0.0, 7)
    assert got.tolist() == [1, 4, 0, 2]                                # a key of 0 is not above 0
    got, s = check_threshold(mrt_mod, "no pixels", [np.inf, 1.0, np.nan], [0, 0, 0], 0.5, 3)
    assert got.tolist() == [] and s == {"frame_error": 0.0, "max_tile_error": 0.0, "tiles_above": 0,
                                        "tiles_listed": 0, "tiles_counted": 0, "pixels": 0}


@pytest.mark.parametrize("T,quantile,max_count", [(1000, 0.7, 100), (1000, 0.7, 1000), (1000, 0.7, 300), (1000, 2.0, 1000),
                                                  (16384, 0.9, 16384), (16384, 0.5, 5)])
def test_tile_threshold_large(gpu, mrt_mod, T, quantile, max_count):
    """max_count below, at and above A; A = 0 (quantile 2: a threshold above every key); every block count."""
    e, n = random_tiles(T, T + max_count)
    if T == 16384:
        e[::3] = e[1]                                                  # thousands of ties, broken by tile index
    key = np.where(n > 0, e, 0)
    threshold = float(np.quantile(key, quantile)) if quantile <= 1 else float(key.max())
    if max_count == 300:
        threshold = float(np.sort(key)[T - 301])                       # the 301st largest key: 300 above it
    got, s = check_threshold(mrt_mod, f"T={T} max_count={max_count}", e, n, threshold, max_count)
    A = int((key > np.float32(threshold)).sum())
    assert s["tiles_above"] == A and len(got) == min(A, max_count) and len(set(got.tolist())) == len(got)
    if quantile > 1:
        assert A == 0
    elif (T, max_count) == (1000, 100):
        assert A > max_count
    elif (T, max_count) == (1000, 1000):
        assert 0 < A < max_count
    elif (T, max_count) == (1000, 300):
        assert A == 300                                                # exactly as many as fit


def test_tile_threshold_argument_errors(gpu, mrt_mod):
    d_e, d_n = to_dev(np.ones(16385, np.float32)), to_dev(np.ones(16385, np.uint32))
    d_l, d_s = to_dev(np.zeros(16385, np.uint32)), to_dev(np.zeros(8, np.uint32))
    E, N, Lp, S = dev_ptr(d_e), dev_ptr(d_n), dev_ptr(d_l), dev_ptr(d_s)
    call = mrt_mod.tile_threshold
    for T, K in [(16385, 1), (0, 1), (8, 0), (8, 9)]:
        assert status_of(mrt_mod, call, E, N, T, 0.5, K, Lp, S) == ERR_INVALID, (T, K)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert status_of(mrt_mod, call, E, N, 8, bad, 8, Lp, S) == ERR_INVALID, bad
    overlaps = [(E, E + 16, Lp, S), (E, N, E + 16, S), (E, N, N + 16, S), (E, N, Lp, E + 4), (E, N, Lp, N),
                (E, N, Lp, Lp + 8), (E, N, S, S)]
    for e, n, l, s in overlaps:
        assert status_of(mrt_mod, call, e, n, 8, 0.5, 8, l, s) == ERR_INVALID
    for e, n, l, s in [(None, N, Lp, S), (E, None, Lp, S), (E, N, None, S), (E, N, Lp, None)]:
        assert status_of(mrt_mod, call, e, n, 8, 0.5, 8, l, s) == ERR_INVALID
    assert not from_dev(d_l, np.uint32).any() and not from_dev(d_s, np.uint32).any()
    call(E, N, 16384, 0.0, 16384, Lp, S)                                # the largest frame: every tile above, in order
    assert (from_dev(d_l, np.uint32)[:16384] == np.arange(16384)).all()


# ---- the renderer against the stage pipeline ----------------------------------------
def stage_estimate(st, resolved, moments, g, threshold, eps=0.01):
    """What mrt_renderer_error does, from the stage calls: (variance, denoised, means, pixels, list, summary)."""
    m, W, H = st.m, st.W, st.H
    T = tiles_of(W, H)[0] * tiles_of(W, H)[1]
    sp = m.SvgfParams.default()
    var, den, scratch = st._buf(1), st._buf(), st._buf()
    m.variance(dev_ptr(moments), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(var), W, H, sp)
    m.denoise_variance(dev_ptr(resolved), dev_ptr(var), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(den), dev_ptr(scratch),
                       None, W, H, sp)
    d_e, d_n = to_dev(np.zeros(T, np.float32)), to_dev(np.zeros(T, np.uint32))
    d_l, d_s = to_dev(np.full(T, 0xFFFFFFFF, np.uint32)), to_dev(np.zeros(8, np.uint32))
    m.tile_error(dev_ptr(den), dev_ptr(var), dev_ptr(g[0]), dev_ptr(d_e), dev_ptr(d_n), W, H, m.AdaptiveParams(eps),
                 precise=st.precise)
    m.tile_threshold(dev_ptr(d_e), dev_ptr(d_n), T, threshold, T, dev_ptr(d_l), dev_ptr(d_s))
    s = m.ErrorSummary.from_buffer_copy(from_dev(d_s, np.uint32).tobytes()).as_dict()
    return (st.host(var, 1)[..., 0], st.host(den), from_dev(d_e, np.float32), from_dev(d_n, np.uint32),
            from_dev(d_l, np.uint32)[:s["tiles_listed"]], s)


@pytest.mark.parametrize("precise", [True, False])
def test_converge_equals_stage_pipeline(gpu, mrt_mod, precise):
    """error_estimate = denoise_variance + the two stage calls; converge = a replay with draw_tiles and the stage
    calls.  Everything the replay computes goes through the same kernels on the same inputs, so both builds
    are compared bit for bit."""
    st = Stage(mrt_mod, precise)
    g = st.guides(None)                                                  # the reference's camera
    mk = lambda: mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise, moments=True)   # noqa: E731
    r, plain, replay = mk(), mk(), mk()
    for x in (r, plain, replay):
        x.draw(8)
    assert status_of(mrt_mod, r.read_tile_error) == ERR_STATE
    s0 = r.error_estimate(0.0)
    img8, mom8 = plain.read_image(), plain.read_moments()
    assert r.read_image().tobytes() == img8.tobytes()
    want = stage_estimate(st, st.resolve(img8, 8), st.resolve(mom8, 8), g, 0.0)
    means, pixels = r.read_tile_error()
    assert r.read_variance().tobytes() == want[0].tobytes() and r.read_denoised().tobytes() == want[1].tobytes()
    assert means.tobytes() == want[2].tobytes() and (pixels == want[3]).all() and s0 == want[5]
    assert (r.read_tile_list() == want[4]).all() and s0["tiles_above"] == s0["tiles_listed"] == 6
    assert r.refine_stats() == {"passes": 0, "extra_frames": 0, "tile_frames": 0, "paths": 0}
    # converge, and its replay: estimate, draw the tiles above, estimate, ...
    target = float(np.median(means))
    F, P = 2, 2
    res = r.converge(target_error=target, frames_per_pass=F, max_passes=P)
    E = EM = None
    first = last = None
    passes = tile_frames = paths = 0
    while True:
        est = stage_estimate(st, st.resolve(img8, 8, extra=E), st.resolve(mom8, 8, extra=EM), g, target)
        last = est[5]
        first = first or last
        if last["tiles_above"] == 0 or passes == P:
            break
        replay.draw_tiles(est[4], F)
        E, EM = replay.read_extra(), replay.read_extra_moments()
        passes, tile_frames = passes + 1, tile_frames + len(est[4]) * F
        paths += int(tile_mask(W0, H0, est[4]).sum()) * F
    assert passes >= 1 and first["tiles_above"] == 3                     # the median of six distinct means
    assert res == {"converged": int(last["tiles_above"] == 0), "passes": passes, "tile_frames": tile_frames,
                   "first": first, "last": last}
    assert r.read_extra().tobytes() == E.tobytes() and r.read_extra_moments().tobytes() == EM.tobytes()
    means, pixels = r.read_tile_error()
    assert means.tobytes() == est[2].tobytes() and (pixels == est[3]).all()
    assert r.read_denoised().tobytes() == est[1].tobytes() and r.read_variance().tobytes() == est[0].tobytes()
    if len(est[4]):
        assert (r.read_tile_list() == est[4]).all()
    else:
        assert status_of(mrt_mod, r.read_tile_list) == ERR_STATE
    assert r.refine_stats() == {"passes": passes, "extra_frames": passes * F, "tile_frames": tile_frames, "paths": paths}
    assert r.refine_stats() == replay.refine_stats()
    # the image and the moments are those of a renderer that never converged, and stay so
    s = r.stats()
    assert s["frame_index"] == 8 and s["paths"] == 8 * W0 * H0 and s["draws"] == 1
    assert r.read_image().tobytes() == img8.tobytes() and r.read_moments().tobytes() == mom8.tobytes()
    r.draw(1)
    plain.draw(1)
    assert r.read_image().tobytes() == plain.read_image().tobytes()
    assert r.read_moments().tobytes() == plain.read_moments().tobytes()
    r.resize(96, 64)
    assert status_of(mrt_mod, r.read_tile_error) == ERR_STATE
    for x in (r, plain, replay):
        x.close()


# ---- the stop rule ------------------------------------------------------------------
def test_stop_rule(gpu, mrt_mod):
    sc = _scene(mrt_mod)
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    assert status_of(mrt_mod, r.converge) == ERR_STATE                   # nothing accumulated
    r.draw(3)
    assert status_of(mrt_mod, r.converge) == ERR_STATE                   # fewer than min_frames = 4, no history
    assert status_of(mrt_mod, r.error_estimate) == ERR_STATE
    sp = mrt_mod.SvgfParams.default()
    sp.min_frames = 3
    assert r.error_estimate(0.0, sp)["tiles_counted"] == 6               # (the caller's own min_frames decides)
    r.draw(5)
    rs = r.refine_stats()
    # a huge target: nothing to do
    res = r.converge(target_error=1e30)
    assert (res["converged"], res["passes"], res["tile_frames"]) == (1, 0, 0) and res["first"] == res["last"]
    assert res["last"]["tiles_above"] == 0 and r.refine_stats() == rs
    # a budget smaller than one pass: nothing drawn, not converged
    res = r.converge(target_error=1e-12, frames_per_pass=4, max_tile_frames=3)
    assert (res["converged"], res["passes"], res["tile_frames"]) == (0, 0, 0) and r.refine_stats() == rs
    assert res["last"]["tiles_above"] == 6
    # a tiny target: max_passes draws of max_tiles tiles, and the loop ends on an estimate
    res = r.converge(target_error=1e-12, frames_per_pass=2, max_passes=3, max_tiles=2)
    assert (res["converged"], res["passes"], res["tile_frames"]) == (0, 3, 3 * 2 * 2)
    assert r.refine_stats()["passes"] == 3 and r.refine_stats()["extra_frames"] == 6
    assert len(r.read_tile_list()) == 6 and res["last"]["tiles_above"] == 6
    # a budget that ends the loop: 5 tile-frames at F = 2 are one pass of 2 tiles, and the 1 left buys nothing
    res = r.converge(target_error=1e-12, frames_per_pass=2, max_tiles=2, max_tile_frames=5)
    assert (res["converged"], res["passes"], res["tile_frames"]) == (0, 1, 4)
    # failed checks change nothing
    rs, E = r.refine_stats(), r.read_extra()
    for field, bad in (("target_error", 0.0), ("frames_per_pass", 0), ("max_passes", 0), ("luminance_floor", float("nan"))):
        with pytest.raises(mrt_mod.MrtError, match=field):
            r.converge(**{field: bad})
    assert status_of(mrt_mod, r.error_estimate, -1.0) == ERR_INVALID
    assert status_of(mrt_mod, r.error_estimate, float("nan")) == ERR_INVALID
    assert r.refine_stats() == rs and r.read_extra().tobytes() == E.tobytes()
    assert mrt_mod.lib().mrt_renderer_converge(r._h, None, None) == ERR_INVALID
    assert mrt_mod.lib().mrt_renderer_error(r._h, None, 0.0, 0.0, None) == ERR_INVALID
    r.close()
    for kw in ({}, {"shard_count": 2}, {"moments": True, "animate_noise": False}):
        r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, **kw)
        r.draw(8)
        assert status_of(mrt_mod, r.converge) == ERR_STATE, kw
        assert status_of(mrt_mod, r.error_estimate) == ERR_STATE, kw
        assert status_of(mrt_mod, r.read_tile_error) == ERR_STATE, kw
        r.close()


def test_converge_behaviour(gpu, mrt_mod):
    """192x128, the fast build: 8 frames, then to half of the worst tile's error at 8 frames per pass."""
    r = mrt_mod.Renderer(_scene(mrt_mod), 192, 128, L0, precise=False, moments=True)
    r.draw(8)
    first = r.error_estimate(0.0)
    target = 0.5 * first["max_tile_error"]
    res = r.converge(target_error=target, frames_per_pass=8)
    means, _ = r.read_tile_error()
    E = r.read_extra()
    counts = [float(E[tile_mask(192, 128, [t]).astype(bool)][0, 3]) for t in range(6)]
    print(f"target {target:.5g}: {res['passes']} passes, {res['tile_frames']} tile-frames, frame error "
          f"{res['first']['frame_error']:.5g} -> {res['last']['frame_error']:.5g}, extra frames per tile {counts}, "
          f"tile means {means.tolist()}")
    assert res["converged"] == 1 and res["passes"] >= 1
    assert res["last"]["max_tile_error"] <= np.float32(target) and (means <= np.float32(target)).all()
    assert len(set(counts)) > 1 and min(counts) == 0                     # the samples went where the error was
    assert res["first"]["frame_error"] == first["frame_error"] and res["last"]["frame_error"] < first["frame_error"]
    assert sum(counts) == res["tile_frames"]
    r.close()


def test_cli_target_error(gpu, mrt_mod, tmp_path):
    """mrt_render --target-error writes the Python path's denoised image and prints the line."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    base = [exe, "--scene", "cornellbox", "--w", "64", "--h", "48", "--spp", "8", "--L", "4", "--precise"]
    r = mrt_mod.Renderer(_scene(mrt_mod), 64, 48, 4, precise=True, moments=True)
    r.draw(8)
    target = 0.5 * r.error_estimate(0.0)["max_tile_error"]
    res = r.converge(target_error=target, frames_per_pass=4, max_passes=5)
    want = np.ascontiguousarray(r.read_denoised()[..., :3]).tobytes()
    r.close()
    out = tmp_path / "a.pfm"
    p = subprocess.run(base + ["--target-error", repr(float(target)), "--converge-frames", "4", "--converge-max-passes", "5",
                               "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    line = json.loads(next(ln for ln in p.stdout.splitlines() if "converge_passes" in ln))
    assert line["converge_passes"] == res["passes"] >= 1 and line["tile_frames"] == res["tile_frames"]
    assert line["converged"] == res["converged"]
    assert np.float32(line["first_frame_error"]) == np.float32(res["first"]["frame_error"])
    assert np.float32(line["last_frame_error"]) == np.float32(res["last"]["frame_error"])
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert (w, h) == (64, 48) and float(f.readline()) < 0
        assert np.frombuffer(f.read(), "<f4").tobytes() == want
    for extra, msg in ((["--target-error", "0.1", "--refine-passes", "1"], "exclude"),
                       (["--target-error", "0.1", "--gpus", "2"], "single rank"),
                       (["--converge-frames", "2"], "--target-error")):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, extra
