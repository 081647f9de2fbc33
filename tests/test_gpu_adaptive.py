"""Adaptive sampling on the device (include/mrt.h "adaptive sampling", DESIGN.md
§2.1q): the tile list in the render kernels and the counted accumulate against
the oracle, bit for bit in the precise build; the stage calls mrt_counted_merge,
mrt_tile_priority and mrt_tile_select against tests/adaptive_model.py; the
renderer layer (refine, the merged resolves, the readers, the CLI) against the
stage pipeline.

Tolerances: the precise build's extra images and merge are compared bit for bit
and the selection is exact.  The fast build's extra image is held to the gate of
test_gpu_parity.test_render_parity_fast; the fast merge and both builds'
priority (its summation order is free) to the rule of test_gpu_denoise.py: four
times the largest deviation of the float32 model from the float64 model on the
same inputs, computed and printed per case."""
import os
import subprocess

import numpy as np
import pytest

from adaptive_model import TILE, counted_merge, tile_mask, tile_pixels, tile_priority, tile_select, tiles_of
from camera_cases import camera
from helpers import SEED, dev_ptr, from_dev, pixel_metrics, to_dev
from variance_model import moments_records

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5
W0, H0, L0 = 160, 96, 4          # 3 x 2 tiles: the right column 32 px wide, the top row 32 px tall


def _scene(mrt_mod, name="cornellbox", cache={}):
    if name not in cache:
        cache[name] = mrt_mod.Scene(name)
    return cache[name]


def _oscene(oracle_mod, mrt_mod, name, cache={}):
    if name not in cache:
        cache[name] = oracle_mod.OracleScene(mrt_mod.scene_path(name))
    return cache[name]


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


# ---- list decode and counted accumulate ----------------------------------------
def expected_extras(oracle_mod, mrt_mod, scene, W, H, L, passes):
    """E and EM after the refine draws `passes` = [(tiles, frames), ...] from extra frame 0: the oracle's
    per-frame radiance with the refine seed, folded per tile at the tile's own count."""
    osc = _oscene(oracle_mod, mrt_mod, scene)
    E, EM = np.zeros((H * W, 4), np.float32), np.zeros((H * W, 4), np.float32)
    e = 0
    for tiles, frames in passes:
        mask = tile_mask(W, H, tiles)
        idx = np.flatnonzero(mask.reshape(-1))
        for _ in range(frames):
            rad, _ = osc.render(W, H, L, SEED ^ mrt_mod.REFINE_SEED_XOR, 1, frame_begin=e, threads=8,
                                pixel_mask=mask, flags=oracle_mod.NO_ACCUMULATE)
            rgb = np.ascontiguousarray(rad.reshape(-1, 4)[:, :3])
            for t in tiles:
                ti = np.flatnonzero(tile_mask(W, H, [t]).reshape(-1))
                n = int(E[ti[0], 3])
                rays = np.zeros(len(ti), oracle_mod.RAY_DTYPE)
                rays["radiance"][:, :3] = rgb[ti]
                for img, rec in ((E, rays), (EM, moments_records(oracle_mod, rgb[ti]))):
                    part = np.ascontiguousarray(img[ti])
                    oracle_mod.accumulate(n, rec, part)
                    part[:, 3] = n + 1
                    img[ti] = part
            e += 1
        assert len(idx) == sum(tile_pixels(W, H, t) for t in tiles)
    return E.reshape(H, W, 4), EM.reshape(H, W, 4)


SEQ = [([5, 0, 3], 3), ([3, 1], 2)]


def test_draw_tiles_precise_stream_kernel(gpu, mrt_mod, oracle_mod):
    sc = _scene(mrt_mod)
    plain = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    plain.draw(2)
    img2, mom2 = plain.read_image(), plain.read_moments()
    plain.draw(2)
    img4, mom4 = plain.read_image(), plain.read_moments()
    plain.close()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    assert r.stats()["kernel"] == 2
    assert status_of(mrt_mod, r.read_extra) == ERR_STATE and status_of(mrt_mod, r.read_tile_list) == ERR_STATE
    r.draw(2)
    for tiles, frames in SEQ:
        r.draw_tiles(tiles, frames)
    E, EM = r.read_extra(), r.read_extra_moments()
    wantE, wantEM = expected_extras(oracle_mod, mrt_mod, "cornellbox", W0, H0, L0, SEQ)
    counts = {0: 3, 1: 2, 2: 0, 3: 5, 4: 0, 5: 3}
    for t, n in counts.items():
        m = tile_mask(W0, H0, [t]).astype(bool)
        assert (E[m][:, 3] == n).all() and (EM[m][:, 3] == n).all(), t
        if n == 0:
            assert not E[m].any() and not EM[m].any()
    assert E.tobytes() == wantE.tobytes()
    assert EM.tobytes() == wantEM.tobytes()
    assert E[..., :3].max() > 0.1 and (EM[..., 2] == 0).all()
    assert (r.read_tile_list() == [3, 1]).all()
    # the image and the moments are those of a renderer that never drew tiles, and stay so
    assert r.read_image().tobytes() == img2.tobytes() and r.read_moments().tobytes() == mom2.tobytes()
    r.draw(2)
    assert r.read_image().tobytes() == img4.tobytes() and r.read_moments().tobytes() == mom4.tobytes()
    st, rs = r.stats(), r.refine_stats()
    assert st["frame_index"] == 4 and st["paths"] == 4 * W0 * H0 and st["draws"] == 2
    assert rs == {"passes": 2, "extra_frames": 5, "tile_frames": 13,
                  "paths": 3 * sum(tile_pixels(W0, H0, t) for t in (5, 0, 3)) + 2 * sum(tile_pixels(W0, H0, t) for t in (3, 1))}
    r.close()


def test_draw_tiles_precise_path_kernel(gpu, mrt_mod, oracle_mod):
    W, H = 96, 64
    r = mrt_mod.Renderer(_scene(mrt_mod, "CornellBox-Water"), W, H, L0, precise=True, moments=True)
    assert r.stats()["kernel"] == 1
    r.draw(1)
    img = r.read_image()
    r.draw_tiles([1], 2)
    wantE, wantEM = expected_extras(oracle_mod, mrt_mod, "CornellBox-Water", W, H, L0, [([1], 2)])
    assert r.read_extra().tobytes() == wantE.tobytes() and r.read_extra_moments().tobytes() == wantEM.tobytes()
    assert r.read_image().tobytes() == img.tobytes()
    r.close()


@pytest.mark.parametrize("cam", ["A", "E"])
def test_draw_tiles_all_tiles_is_a_draw_with_the_refine_seed(gpu, mrt_mod, cam):
    """With a moved camera (A) and a thin lens (E): E after draw_tiles(all tiles, 2) is bitwise the image of a
    fresh renderer with the refine seed and that camera after draw(2)."""
    c = camera(mrt_mod, cam)
    assert (c.lens_radius > 0) == (cam == "E")
    sc = _scene(mrt_mod)
    fresh = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, seed=SEED ^ mrt_mod.REFINE_SEED_XOR)
    fresh.set_camera(c)
    fresh.draw(2)
    want = fresh.read_image()
    fresh.close()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    r.set_camera(c)
    r.draw_tiles([4, 2, 0, 5, 1, 3], 2)
    E = r.read_extra()
    assert E[..., :3].tobytes() == want[..., :3].tobytes() and (E[..., 3] == 2).all()
    r.close()


def test_draw_tiles_fast_against_precise(gpu, mrt_mod):
    out = {}
    for precise in (True, False):
        r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise, moments=True)
        r.draw(2)
        for tiles, frames in SEQ:
            r.draw_tiles(tiles, frames)
        out[precise] = r.read_extra()
        r.close()
    assert out[False][..., 3].tobytes() == out[True][..., 3].tobytes()
    drawn = out[True][..., 3] > 0
    rel, rmse, same = pixel_metrics(out[False][drawn][None], out[True][drawn][None])
    print(f"fast E against precise E: bit-identical {same:.4f}, rel<=1e-2 {np.mean(rel <= 1e-2):.5f}, rmse {rmse:.2e}")
    assert np.mean(rel <= 1e-2) >= 0.99          # the gate of test_gpu_parity.test_render_parity_fast
    assert not out[False][~drawn].any()


# ---- mrt_counted_merge ------------------------------------------------------------
def merge_inputs(W, H, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 3.0, size=(H, W, 4)).astype(np.float32)
    b = rng.uniform(0.0, 3.0, size=(H, W, 4)).astype(np.float32)
    a[..., 3] = rng.integers(0, 6, size=(H, W))
    b[..., 3] = rng.integers(0, 6, size=(H, W))
    if W * H >= 16:   # the four bitwise branches, each at a known pixel
        fa, fb = a.reshape(-1, 4), b.reshape(-1, 4)
        fb[0] = (1.5, np.nan, 0.25, 0.0)      # hb == 0: a, whatever b holds
        fa[0, 3] = 2.0
        fb[1] = (np.inf, 1.0, 1.0, 3.0)       # b not finite: a
        fa[1] = (0.5, 0.25, 0.125, 0.0)       # ... even an empty a
        fa[2] = (-0.0, 7.0, np.nan, 0.0)      # ha == 0: b
        fb[2, 3] = 4.0
        fa[3] = (np.nan, 1.0, 1.0, 2.0)       # a not finite: b
        fb[3, 3] = 1.0
        fa[4, 3], fb[4, 3] = 3.0, 2.0         # both: the weighted mean
    return a, b


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("W,H", [(53, 37), (1, 1)])
def test_counted_merge(gpu, mrt_mod, W, H, precise):
    a, b = merge_inputs(W, H, 10 * W + H)
    if W == 1:
        a[0, 0], b[0, 0] = (0.5, 1.5, 2.5, 3.0), (1.0, 0.25, 0.125, 2.0)
    m32, m64 = counted_merge(a, b, np.float32), counted_merge(a, b, np.float64)
    d_a, d_b, d_o = to_dev(a), to_dev(b), to_dev(np.full_like(a, -7.0))
    mrt_mod.counted_merge(dev_ptr(d_a), dev_ptr(d_b), dev_ptr(d_o), W, H, precise=precise)
    got = from_dev(d_o, np.float32).reshape(H, W, 4)
    assert from_dev(d_a, np.float32).tobytes() == a.tobytes() and from_dev(d_b, np.float32).tobytes() == b.tobytes()
    copies = (b[..., 3] == 0) | ~np.isfinite(b[..., :3]).all(-1) | (a[..., 3] == 0) | ~np.isfinite(a[..., :3]).all(-1)
    assert got[copies].tobytes() == m32[copies].tobytes()                 # the bitwise branches, in both builds
    if W > 1:
        assert copies.reshape(-1)[:4].all() and not copies.reshape(-1)[4]
        assert got.reshape(-1, 4)[0].tobytes() == a.reshape(-1, 4)[0].tobytes()
        assert got.reshape(-1, 4)[2].tobytes() == b.reshape(-1, 4)[2].tobytes()
    if precise:
        assert got.tobytes() == m32.tobytes()
    else:
        within(f"mrt_counted_merge {W}x{H}, fast build", got[~copies], m64[~copies], m32[~copies])
    mrt_mod.counted_merge(dev_ptr(d_a), dev_ptr(d_b), dev_ptr(d_a), W, H, precise=precise)   # out == a
    assert from_dev(d_a, np.float32).tobytes() == got.tobytes()


def test_counted_merge_overlap_errors(gpu, mrt_mod):
    n = 53 * 37 * 4
    a, b, o = (to_dev(np.zeros(n + 64, np.float32)) for _ in range(3))
    call = lambda *p: mrt_mod.counted_merge(*p, 53, 37)   # noqa: E731
    pa, pb, po = dev_ptr(a), dev_ptr(b), dev_ptr(o)
    for args in [(pa, pb, pb), (pa, pb, pb + 16), (pa, pb, pa + 16), (pa + 16, pb, pa), (pa, pa, pa)]:
        assert status_of(mrt_mod, call, *args) == ERR_INVALID, args
    assert status_of(mrt_mod, call, pa, None, po) == ERR_INVALID
    call(pa, pb, po)
    call(pa, pb, pa)


# ---- mrt_tile_priority ------------------------------------------------------------
def rendered_planes(mrt_mod, W, H, cache={}):
    """(resolved image, variance plane, guide normals) of a 3-frame render at W x H, with a light visible."""
    if (W, H) not in cache:
        r = mrt_mod.Renderer(_scene(mrt_mod), max(W, 2), max(H, 2), L0, moments=True)
        r.draw(3)
        r.denoise_variance()
        img, var = r.read_resolved()[:H, :W].copy(), r.read_variance()[:H, :W].copy()
        r.close()
        gn, gp = to_dev(np.zeros((max(H, 2), max(W, 2), 4), np.float32)), to_dev(np.zeros((max(H, 2), max(W, 2), 4), np.float32))
        mrt_mod.guides(_scene(mrt_mod), max(W, 2), max(H, 2), dev_ptr(gn), dev_ptr(gp), precise=False)
        g = from_dev(gn, np.float32).reshape(max(H, 2), max(W, 2), 4)[:H, :W].copy()
        cache[(W, H)] = (np.ascontiguousarray(img), np.ascontiguousarray(var), np.ascontiguousarray(g))
    return cache[(W, H)]


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("W,H", [(160, 96), (65, 1), (64, 64)])
def test_tile_priority(gpu, mrt_mod, W, H, precise):
    img, var, gn = (v.copy() for v in rendered_planes(mrt_mod, W, H))
    if W * H > 200:
        img[H // 2, W // 3, 1] = np.nan          # a non-finite pixel is left out
    p = mrt_mod.AdaptiveParams.default()
    tx, ty = tiles_of(W, H)
    d = [to_dev(v) for v in (img, var, gn)]
    d_p = to_dev(np.full(tx * ty, -3.0, np.float32))
    mrt_mod.tile_priority(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_p), W, H, p, precise=precise)
    got = from_dev(d_p, np.float32)
    m64 = tile_priority(img, var, gn, p.luminance_floor, np.float64)
    m32 = tile_priority(img, var, gn, p.luminance_floor, np.float32)
    assert np.isfinite(m64).all() and (got >= 0).all() and m64.max() > 0
    # relative to each tile's own sum: the sums of different tiles differ by orders of magnitude
    scale = np.maximum(m64, 1e-30)
    within(f"mrt_tile_priority {W}x{H} {'precise' if precise else 'fast'}", got / scale, m64 / scale,
           (m32.astype(np.float64) / scale))
    assert (got[m64 == 0] == 0).all()
    for k, t in enumerate(d[:3]):
        assert from_dev(t, np.float32).tobytes() == (img, var, gn)[k].tobytes()


def test_tile_priority_empty_tile_and_errors(gpu, mrt_mod):
    W, H = 160, 96
    img, var, gn = (v.copy() for v in rendered_planes(mrt_mod, W, H))
    gn[:64, 64:128, 3] = np.uint32(0xFFFFFFFF).view(np.float32)      # tile 1: no filterable pixel
    p = mrt_mod.AdaptiveParams.default()
    d = [to_dev(v) for v in (img, var, gn)]
    d_p = to_dev(np.full(6, -3.0, np.float32))
    call = lambda *a: mrt_mod.tile_priority(*a[:4], W, H, *a[4:])   # noqa: E731
    call(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_p), p)
    got = from_dev(d_p, np.float32)
    assert got[1] == 0 and (got[[0, 2, 3, 4, 5]] > 0).all()
    assert status_of(mrt_mod, call, dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_p), None) == ERR_INVALID
    for t in d:
        assert status_of(mrt_mod, call, dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(t) + 8, p) == ERR_INVALID
    bad = mrt_mod.AdaptiveParams(0.0)
    with pytest.raises(mrt_mod.MrtError, match="luminance_floor"):
        call(dev_ptr(d[0]), dev_ptr(d[1]), dev_ptr(d[2]), dev_ptr(d_p), bad)


# ---- mrt_tile_select ----------------------------------------------------------------
def gpu_select(mrt_mod, pri, K):
    pri = np.ascontiguousarray(pri, np.float32)
    d_p, d_l = to_dev(pri), to_dev(np.full(max(K, 1) + 2, 0xFFFFFFFF, np.uint32))
    mrt_mod.tile_select(dev_ptr(d_p), len(pri), K, dev_ptr(d_l))
    out = from_dev(d_l, np.uint32)
    assert (out[K:] == 0xFFFFFFFF).all()             # nothing behind the list is written
    return out[:K]


def spaced(T, seed):
    """T priorities spaced at least 10 % apart, shuffled."""
    p = (1.1 ** np.arange(T, dtype=np.float64) * 1e-20) if T > 600 else (1.1 ** np.arange(T, dtype=np.float64))
    p = p[p < 3e38][:T]
    assert len(p) == T
    return np.random.default_rng(seed).permutation(p).astype(np.float32)


@pytest.mark.parametrize("T,K", [(1, 1), (7, 3), (1000, 1), (1000, 999), (1000, 1000), (16384, 5)])
def test_tile_select(gpu, mrt_mod, T, K):
    if T == 7:
        pri = np.array([2.0, 5.0, 2.0, -1.0, 5.0, np.nan, 2.0], np.float32)     # ties, a negative, a NaN
        assert (tile_select(pri, 3) == [1, 4, 0]).all()
    elif T == 16384:
        # more values than a float32 holds 10 % apart: 1000 spaced ones among equal (tied) ones
        pri = np.full(T, 0.5, np.float32)
        pos = np.random.default_rng(3).choice(T, 1000, replace=False)
        pri[pos] = spaced(1000, 4) + np.float32(1.0)
    else:
        pri = spaced(T, T + K)
    want = tile_select(pri, K)
    got = gpu_select(mrt_mod, pri, K)
    assert (got == want).all()
    assert len(set(got.tolist())) == K
    if K == T:
        assert sorted(got.tolist()) == list(range(T))               # no tile is exempt


def test_tile_select_equal_and_bad_priorities(gpu, mrt_mod):
    assert (gpu_select(mrt_mod, np.full(300, 0.25, np.float32), 300) == np.arange(300)).all()
    pri = np.array([-np.inf, np.inf, -2.0, 0.0, np.nan, 1e-30], np.float32)   # only the last one is above 0
    assert (gpu_select(mrt_mod, pri, 6) == [5, 0, 1, 2, 3, 4]).all()
    d_p, d_l = to_dev(np.zeros(16385, np.float32)), to_dev(np.zeros(16385, np.uint32))
    for T, K in [(16385, 1), (8, 0), (8, 9)]:
        assert status_of(mrt_mod, mrt_mod.tile_select, dev_ptr(d_p), T, K, dev_ptr(d_l)) == ERR_INVALID
    assert status_of(mrt_mod, mrt_mod.tile_select, dev_ptr(d_p), 8, 4, dev_ptr(d_p) + 16) == ERR_INVALID
    mrt_mod.tile_select(dev_ptr(d_p), 16384, 16384, dev_ptr(d_l))
    assert (from_dev(d_l, np.uint32)[:16384] == np.arange(16384)).all()


# ---- refine end to end -----------------------------------------------------------
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

    def resolve(self, img, frames, hist=None, extra=None):
        d_img, out = to_dev(img), self._buf()
        self.m.temporal_resolve(dev_ptr(d_img), frames, dev_ptr(hist) if hist is not None else None, dev_ptr(out),
                                self.W, self.H)
        if extra is not None:
            d_e = to_dev(extra)
            self.m.counted_merge(dev_ptr(out), dev_ptr(d_e), dev_ptr(out), self.W, self.H, precise=self.precise)
        return out

    def reproject(self, prev, g_prev, cam_prev, g_cur):
        out = self._buf()
        self.m.reproject(dev_ptr(prev), dev_ptr(g_prev[0]), dev_ptr(g_prev[1]), cam_prev, dev_ptr(g_cur[0]),
                         dev_ptr(g_cur[1]), dev_ptr(out), self.W, self.H, self.m.ReprojectParams.default())
        return out

    def choose(self, resolved, moments, g, K):
        """(variance, priorities, list) of the stage calls on resolved colour and moments."""
        tx, ty = tiles_of(self.W, self.H)
        var, pri, lst = self._buf(1), to_dev(np.zeros(tx * ty, np.float32)), to_dev(np.zeros(tx * ty, np.uint32))
        self.m.variance(dev_ptr(moments), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(var), self.W, self.H,
                        self.m.SvgfParams.default())
        self.m.tile_priority(dev_ptr(resolved), dev_ptr(var), dev_ptr(g[0]), dev_ptr(pri), self.W, self.H,
                             self.m.AdaptiveParams.default(), precise=self.precise)
        self.m.tile_select(dev_ptr(pri), tx * ty, K, dev_ptr(lst))
        return self.host(var, 1)[..., 0], from_dev(pri, np.float32), from_dev(lst, np.uint32)[:K]

    def host(self, t, c=4):
        return from_dev(t, np.float32).reshape(self.H, self.W, c)


@pytest.mark.parametrize("precise", [True, False])
def test_refine_equals_stage_pipeline(gpu, mrt_mod, precise):
    st = Stage(mrt_mod, precise)
    A, D = camera(mrt_mod, "A"), camera(mrt_mod, "D")
    gA, gD = st.guides(A), st.guides(D)
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=precise, moments=True)
    r.set_camera(A)
    assert status_of(mrt_mod, r.refine, 2, 2) == ERR_STATE            # nothing accumulated, no history
    assert status_of(mrt_mod, r.read_tile_priority) == ERR_STATE
    r.draw(4)
    r.refine(2, 2)                   # enqueued behind the draw, no sync in between
    pri, lst = r.read_tile_priority(), r.read_tile_list()
    img4, mom4 = r.read_image(), r.read_moments()
    res4, mres4 = st.resolve(img4, 4), st.resolve(mom4, 4)
    want_var, want_pri, want_lst = st.choose(res4, mres4, gA, 2)
    assert pri.tobytes() == want_pri.tobytes() and (lst == want_lst).all()
    assert r.read_variance().tobytes() == want_var.tobytes()
    assert (lst == tile_select(pri, 2)).all() and (pri > 0).all()     # the exact top 2 of what was read back
    E, EM = r.read_extra(), r.read_extra_moments()
    chosen = tile_mask(W0, H0, lst).astype(bool)
    assert (E[chosen][:, 3] == 2).all() and not E[~chosen].any()
    assert (EM[chosen][:, 3] == 2).all() and not EM[~chosen].any()
    r.resolve()
    res = r.read_resolved()
    assert (res[chosen][:, 3] == 6).all() and (res[~chosen][:, 3] == 4).all()
    assert res.tobytes() == st.host(st.resolve(img4, 4, extra=E)).tobytes()
    assert res[~chosen].tobytes() == st.host(res4)[~chosen].tobytes()
    rs = r.refine_stats()
    assert rs == {"passes": 1, "extra_frames": 2, "tile_frames": 4, "paths": 2 * int(chosen.sum())}
    s = r.stats()
    assert s["frame_index"] == 4 and s["paths"] == 4 * W0 * H0 and s["draws"] == 1
    assert r.read_image().tobytes() == img4.tobytes() and r.read_moments().tobytes() == mom4.tobytes()
    # a second pass sees the extra samples: its inputs are the merged images
    r.refine(2, 6)
    want_var, want_pri, want_lst = st.choose(st.resolve(img4, 4, extra=E), st.resolve(mom4, 4, extra=EM), gA, 6)
    assert r.read_tile_priority().tobytes() == want_pri.tobytes() and (r.read_tile_list() == want_lst).all()
    E2, EM2 = r.read_extra(), r.read_extra_moments()
    assert (E2[chosen][:, 3] == 4).all() and (E2[~chosen][:, 3] == 2).all()
    assert r.refine_stats()["extra_frames"] == 4 and r.refine_stats()["tile_frames"] == 16
    # denoise_variance filters the merged image
    r.denoise_variance()
    assert r.read_resolved().tobytes() == st.host(st.resolve(img4, 4, extra=E2)).tobytes()
    # a move carries the merged images into the history and clears the extras
    r.move_camera(D)
    assert not r.read_extra().any() and not r.read_extra_moments().any()
    hist = st.reproject(st.resolve(img4, 4, extra=E2), gA, A, gD)
    mhist = st.reproject(st.resolve(mom4, 4, extra=EM2), gA, A, gD)
    r.draw(2)
    r.refine(1, 3)
    img2, mom2 = r.read_image(), r.read_moments()
    want_var, want_pri, want_lst = st.choose(st.resolve(img2, 2, hist), st.resolve(mom2, 2, mhist), gD, 3)
    assert r.read_tile_priority().tobytes() == want_pri.tobytes() and (r.read_tile_list() == want_lst).all()
    assert r.refine_stats()["extra_frames"] == 5
    # reset clears the extras; the counter keeps running
    r.reset()
    r.draw(1)
    r.resolve()
    assert (r.read_resolved()[..., 3] == 1).all() and not r.read_extra().any()
    r.refine(1, 1)
    assert r.refine_stats()["extra_frames"] == 6 and r.refine_stats()["passes"] == 4
    r.resize(96, 64)
    assert status_of(mrt_mod, r.read_extra) == ERR_STATE and status_of(mrt_mod, r.read_tile_priority) == ERR_STATE
    r.draw(2)
    r.refine(1, 1)
    assert r.read_extra().shape == (64, 96, 4) and r.refine_stats()["extra_frames"] == 7
    r.close()


def test_refine_state_and_argument_errors(gpu, mrt_mod):
    sc = _scene(mrt_mod)
    for kw in ({}, {"shard_count": 2}, {"moments": True, "animate_noise": False}):
        r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, **kw)
        r.draw(1)
        assert status_of(mrt_mod, r.refine, 1, 1) == ERR_STATE, kw
        assert status_of(mrt_mod, r.draw_tiles, [0], 1) == ERR_STATE, kw
        assert status_of(mrt_mod, r.read_extra) == ERR_STATE
        r.close()
    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    assert status_of(mrt_mod, r.refine, 1, 1) == ERR_STATE            # no frame accumulated
    r.draw(1)
    r.draw_tiles([2], 1)
    E, rs = r.read_extra(), r.refine_stats()
    for bad in ([1, 1], [6], [0, 1, 2, 3, 4, 5, 0], []):
        assert status_of(mrt_mod, r.draw_tiles, bad, 1) == ERR_INVALID, bad
    assert status_of(mrt_mod, r.draw_tiles, [0], 0) == ERR_INVALID
    for frames, K in ((0, 1), (1, 0), (1, 7)):
        assert status_of(mrt_mod, r.refine, frames, K) == ERR_INVALID
    with pytest.raises(mrt_mod.MrtError, match="luminance_floor"):
        r.refine(1, 1, mrt_mod.AdaptiveParams(-1.0))
    assert r.read_extra().tobytes() == E.tobytes() and r.refine_stats() == rs and (r.read_tile_list() == [2]).all()
    r.close()


def test_cli_refine(gpu, mrt_mod, tmp_path):
    """mrt_render --refine-passes 2 --refine-frames 2 --refine-tiles 2 --denoise-variance writes the Python path's image."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    base = [exe, "--scene", "cornellbox", "--w", "160", "--h", "96", "--spp", "2", "--L", "4", "--precise"]

    def run(extra, name):
        out = tmp_path / name
        p = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF"
            w, h = map(int, f.readline().split())
            assert (w, h) == (160, 96) and float(f.readline()) < 0
            return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)

    rgb = lambda a: np.ascontiguousarray(a[..., :3]).tobytes()   # noqa: E731
    r = mrt_mod.Renderer(_scene(mrt_mod), 160, 96, 4, precise=True, moments=True)
    r.draw(2)
    plain = r.read_image()
    r.refine(2, 2)
    r.refine(2, 2)
    r.resolve()
    res = r.read_resolved()
    r.denoise_variance()
    refine = ["--refine-passes", "2", "--refine-frames", "2", "--refine-tiles", "2"]
    assert run(refine + ["--denoise-variance"], "a.pfm").tobytes() == rgb(r.read_denoised())
    got = run(refine, "b.pfm")
    assert got.tobytes() == rgb(res) and got.tobytes() != rgb(plain)
    r.close()
    p = subprocess.run(base + refine + ["--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "single rank" in p.stderr
