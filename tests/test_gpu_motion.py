"""Moving geometry on the GPU (include/mrt.h): mrt_guides_motion against the
stage pipeline and tests/denoise_model.py guides_from_hits on the PREVIOUS
scene's vertices, mrt_reproject fed the motion planes against
tests/temporal_model.py, and the renderer layer (mrt_renderer_set_scene,
_move_scene, the CLI's --then-scene) against fresh renderers and the stage
replay guides(A), temporal_resolve, guides_motion(B, A), reproject,
temporal_resolve.  Scene pairs: tests/motion_cases.py.

Measured on an MI355X.  Fast build against the model on its own hits, 64x48 and
37x29: pair (a) max |x| error 1.19e-7, max |n| error 1.79e-7 at both; pair (b)
2.38e-7 and 1.79e-7 at 64x48, 1.19e-7 and 1.79e-7 at 37x29; t and words equal
(bound 2e-5).  mrt_reproject through pair (a)'s motion
planes, float32 model deviation / kernel error (the tolerance is four times the
first): 64x48 1.66e-4 / 1.66e-4 with 40 fragile pixels, 37x29 7.89e-5 / 7.89e-5
with 14; history on 1.000 of the pixels that show the moved box (163 and 53).
Kernel kind (mrt_stats.kernel) on cornellbox 2, on cornellbox + 512 triangles 1."""
import os
import subprocess

import numpy as np
import pytest

from camera_cases import camera
from denoise_model import MISS_WORD, NOT_FILTERABLE, guides_from_hits, words
from helpers import dev_ptr, from_dev, to_dev
from motion_cases import CENTRE, exchanged_obj, moved_obj, mtl_path
from temporal_cases import counted_image, fragile_limit
from temporal_model import reproject

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5
L0 = 4
SIZES = [(64, 48), (37, 29)]     # the second: no tile, block or wave size divides it
_CACHE = {}


def status_of(mrt_mod, fn, *args):
    with pytest.raises(mrt_mod.MrtError) as e:
        fn(*args)
    return e.value.status


def scene(mrt_mod, key, tmp_factory=None):
    """Device scenes, one of each per module: "A" cornellbox, "A2" a second
    object of the same file, "B" pair (a)'s moved copy, ("P", n, seed) cornellbox
    with n procedural triangles (n = 1 << 20: device PLOC, the deep tree)."""
    if key not in _CACHE:
        if key in ("A", "A2"):
            _CACHE[key] = mrt_mod.Scene("cornellbox")
        elif key == "B":
            _CACHE[key] = mrt_mod.Scene(moved_obj(mrt_mod, tmp_factory.mktemp("moved")), mtl_path(mrt_mod))
        else:
            _, n, seed = key
            _CACHE[key] = mrt_mod.Scene("cornellbox", procedural_triangles=n, procedural_seed=seed,
                                        bvh_builder=mrt_mod.BVH_DEVICE_PLOC if n >= 1 << 20 else 0)
    return _CACHE[key]


def export(mrt_mod, key):
    if ("export", key) not in _CACHE:
        _CACHE[("export", key)] = _CACHE[key].export()
    return _CACHE[("export", key)]


def buf(W, H, fill=0.0, c=4):
    return to_dev(np.full((H, W, c), fill, np.float32))


def host(t, W, H, c=4):
    return from_dev(t, np.float32).reshape(H, W, c)


def guide_planes(mrt_mod, sc, W, H, cam=None, precise=True):
    n, p = buf(W, H), buf(W, H)
    mrt_mod.guides(sc, W, H, dev_ptr(n), dev_ptr(p), camera=cam, precise=precise)
    return n, p


def motion_planes(mrt_mod, sc, prev, W, H, cam=None, precise=True):
    """(guide_n, guide_p, motion_n, motion_p) device buffers of mrt_guides_motion"""
    t = [buf(W, H, -7.0) for _ in range(4)]
    mrt_mod.guides_motion(sc, prev, W, H, *(dev_ptr(b) for b in t), camera=cam, precise=precise)
    return t


def stage_hits(mrt_mod, oracle_mod, sc, W, H, cam=None, precise=True):
    d_rays = to_dev(np.zeros(W * H, oracle_mod.RAY_DTYPE))
    mrt_mod.raygen(sc, W, H, dev_ptr(to_dev(CENTRE)), dev_ptr(d_rays), precise=precise, camera=cam)
    d_isect = to_dev(np.zeros(W * H, oracle_mod.ISECT_DTYPE))
    mrt_mod.intersect(sc, dev_ptr(d_rays), 80, W * H, dev_ptr(d_isect), precise=precise)
    return from_dev(d_rays, oracle_mod.RAY_DTYPE), from_dev(d_isect, oracle_mod.ISECT_DTYPE)


# ---- stage level -------------------------------------------------------------
DEEP = 1 << 20
STAGE_CASES = [
    ("B", "A", 64, 48, None),                          # pair (a)
    ("B", "A", 37, 29, None),                          # no tile or block size divides it
    ("B", "A", 32, 32, "B"),                           # from outside: misses
    (("P", 512, 2), ("P", 512, 1), 64, 48, None),      # pair (b)
    (("P", 512, 2), ("P", 512, 1), 37, 29, "A"),
    (("P", DEEP, 2), ("P", DEEP, 1), 32, 32, None),    # pair (c): the spill variant of the traversal stack
    ("A", "A", 64, 48, None),                          # a scene with itself
    ("A", "A2", 37, 29, "A"),                          # ... and with another object of the same file
]


@pytest.mark.parametrize("cur,prev,W,H,cam_name", STAGE_CASES)
def test_guides_motion_precise_bitwise(gpu, mrt_mod, oracle_mod, tmp_path_factory, cur, prev, W, H, cam_name):
    sc, sp = scene(mrt_mod, cur, tmp_path_factory), scene(mrt_mod, prev, tmp_path_factory)
    cam = None if cam_name is None else camera(mrt_mod, cam_name)
    if cur[0] == "P" and cur[1] == DEEP:
        assert sc.info["bvh_max_stack"] > 64, sc.info["bvh_max_stack"]   # the case is about the spill variant
    gn, gp, mn, mp = (host(t, W, H).reshape(-1, 4) for t in motion_planes(mrt_mod, sc, sp, W, H, cam))
    want_n, want_p = (host(t, W, H).reshape(-1, 4) for t in guide_planes(mrt_mod, sc, W, H, cam))
    assert gn.tobytes() == want_n.tobytes() and gp.tobytes() == want_p.tobytes()      # bitwise mrt_guides
    rays, isect = stage_hits(mrt_mod, oracle_mod, sc, W, H, cam)
    model_n, model_p = guides_from_hits(export(mrt_mod, prev), isect, rays)           # the hits in `cur`, `prev`'s vertices
    w = words(gn)
    assert np.array_equal(words(mn), w) and np.array_equal(mp[:, 3], gp[:, 3])
    assert mp.tobytes() == model_p.tobytes()
    assert mn[:, :3].tobytes() == model_n[:, :3].tobytes()
    miss = w == MISS_WORD
    for n_plane, p_plane in ((gn, gp), (mn, mp)):
        assert np.all(n_plane[miss, :3] == 0) and np.all(p_plane[miss, :3] == 0) and np.all(p_plane[miss, 3] == -1.0)
    differ = float(np.mean((mp[:, :3] != gp[:, :3]).any(-1)))
    print(f"{cur} <- {prev} {W}x{H} camera {cam_name}: misses {miss.mean():.3f}, motion differs from guide on {differ:.3f}")
    if cam_name == "B":
        assert miss.any()
    if prev in ("A", "A2") and cur == "A":
        assert mn.tobytes() == gn.tobytes() and mp.tobytes() == gp.tobytes()
    elif cam_name != "B":
        assert differ > 0.02


@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
@pytest.mark.parametrize("cur,prev", [("B", "A"), (("P", 512, 2), ("P", 512, 1))])
def test_guides_motion_fast_build(gpu, mrt_mod, oracle_mod, tmp_path_factory, cur, prev, W, H):
    """Fast build against the model on the fast stage pipeline's own hits: words
    equal, positions and normals within 2e-5 absolute — under four times the
    largest error DESIGN.md §2.1g records for the fast guide planes (5.4e-6).
    Measured: the module's docstring and DESIGN.md §2.1u."""
    sc, sp = scene(mrt_mod, cur, tmp_path_factory), scene(mrt_mod, prev, tmp_path_factory)
    gn, gp, mn, mp = (host(t, W, H).reshape(-1, 4) for t in motion_planes(mrt_mod, sc, sp, W, H, precise=False))
    rays, isect = stage_hits(mrt_mod, oracle_mod, sc, W, H, precise=False)
    model_n, model_p = guides_from_hits(export(mrt_mod, prev), isect, rays)
    own_n, own_p = guides_from_hits(export(mrt_mod, cur), isect, rays)
    err = {name: float(np.abs(got[:, :3].astype(np.float64) - want[:, :3]).max())
           for name, got, want in (("motion x", mp, model_p), ("motion n", mn, model_n), ("guide x", gp, own_p),
                                   ("guide n", gn, own_n))}
    print(f"fast guides_motion {cur} <- {prev} {W}x{H}: " + ", ".join(f"max |{k}| error {v:.3g}" for k, v in err.items()) +
          f", max |t| error {np.abs(mp[:, 3] - model_p[:, 3]).max():.3g}")
    assert np.array_equal(words(mn), words(model_n)) and np.array_equal(words(gn), words(own_n))
    assert np.isfinite(mn[:, :3]).all() and np.isfinite(mp).all()
    assert max(err.values()) <= 2e-5


@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_reproject_through_motion_matches_model(gpu, mrt_mod, tmp_path_factory, W, H):
    """mrt_reproject with pair (a)'s motion planes as the current planes, against
    the float64 model: the comparison, tolerance (four times the float32 model's
    own deviation) and fragile-pixel cap of test_gpu_temporal.py
    test_reproject_matches_model."""
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    params, cam = mrt_mod.ReprojectParams.default(), mrt_mod.Camera.default()
    pn, pp = (host(t, W, H) for t in guide_planes(mrt_mod, A, W, H))
    _, _, d_mn, d_mp = motion_planes(mrt_mod, B, A, W, H)
    cn, cp = host(d_mn, W, H), host(d_mp, W, H)
    prev = counted_image(W, H, 100 * W + H)
    m64, fragile = reproject(prev, pn, pp, cam, cn, cp, params, np.float64)
    m32, _ = reproject(prev, pn, pp, cam, cn, cp, params, np.float32)
    assert fragile.sum() <= fragile_limit(W, H)
    d_out = buf(W, H, -7.0)
    d_prev, d_pn, d_pp = to_dev(prev), to_dev(pn), to_dev(pp)
    mrt_mod.reproject(dev_ptr(d_prev), dev_ptr(d_pn), dev_ptr(d_pp), cam, dev_ptr(d_mn), dev_ptr(d_mp), dev_ptr(d_out),
                      W, H, params)
    got = host(d_out, W, H)
    ok = ~fragile
    dev32 = np.abs(m32[ok].astype(np.float64) - m64[ok]).max()
    err = np.abs(got[ok].astype(np.float64) - m64[ok]).max()
    tol = 4.0 * dev32
    moved = (cp[..., :3] != host(guide_planes(mrt_mod, B, W, H)[1], W, H)[..., :3]).any(-1)   # the pixels that show the block
    print(f"motion {W}x{H}: fragile {fragile.sum()}, history on {np.mean(got[..., 3] > 0):.3f} (on the moved block "
          f"{np.mean(got[..., 3][moved] > 0):.3f} of {moved.sum()}), float32 model deviates {dev32:.3g}, tolerance "
          f"{tol:.3g}, kernel error {err:.3g}")
    assert moved.sum() >= 50
    assert np.isfinite(got).all()
    assert (got[..., 3] >= 0).all() and (got[..., 3] <= params.max_history).all()
    none = got[..., 3] == 0
    assert not got[none].view(np.uint32).any()
    assert not got[words(cn) >= NOT_FILTERABLE].view(np.uint32).any()
    assert np.array_equal(none[ok], m64[..., 3][ok] == 0)
    assert err <= tol
    assert np.mean(got[..., 3][moved] > 0) >= 0.9


def test_guides_motion_argument_errors(gpu, mrt_mod, tmp_path_factory, tmp_path):
    W, H = 16, 8
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    t = [buf(W, H, -7.0) for _ in range(4)]
    p = [dev_ptr(b) for b in t]
    gm = mrt_mod.guides_motion
    water = mrt_mod.Scene("CornellBox-Water")
    exchanged = mrt_mod.Scene(exchanged_obj(mrt_mod, tmp_path), mtl_path(mrt_mod))
    host_only = mrt_mod.Scene("cornellbox", device=-1)
    assert status_of(mrt_mod, gm, B, water, W, H, *p) == ERR_INVALID          # an incompatible pair
    with pytest.raises(mrt_mod.MrtError, match="primitive 4 ") as e:
        gm(B, exchanged, W, H, *p)
    assert e.value.status == ERR_INVALID
    for i in range(4):                                                        # any two planes aliasing
        for j in range(i + 1, 4):
            q = list(p)
            q[j] = q[i]
            assert status_of(mrt_mod, gm, B, A, W, H, *q) == ERR_INVALID, (i, j)
    assert status_of(mrt_mod, gm, B, A, W, H, p[0], p[1], p[2], p[2] + 16) == ERR_INVALID    # overlapping by all but a pixel
    for i in range(4):                                                        # a null plane
        q = list(p)
        q[i] = None
        assert status_of(mrt_mod, gm, B, A, W, H, *q) == ERR_INVALID, i
    L = mrt_mod.lib()
    assert L.mrt_guides_motion(None, A.handle, None, W, H, *p, 1, None) == ERR_INVALID       # a null scene
    assert L.mrt_guides_motion(B.handle, None, None, W, H, *p, 1, None) == ERR_INVALID
    assert status_of(mrt_mod, gm, B, host_only, W, H, *p) == ERR_INVALID     # a host-only scene
    assert status_of(mrt_mod, gm, host_only, A, W, H, *p) == ERR_INVALID
    assert status_of(mrt_mod, gm, B, A, 1, H, *p) == ERR_INVALID             # mrt_guides' own
    bad = mrt_mod.Camera.default()
    bad.tan_half_fov = -1.0
    with pytest.raises(mrt_mod.MrtError, match="tan_half_fov"):
        gm(B, A, W, H, *p, camera=bad)
    for b in t:                                                               # all of them wrote nothing
        assert (host(b, W, H) == -7.0).all()
    gm(B, A, W, H, *p)
    assert all((host(b, W, H) != -7.0).any() for b in t)


# ---- renderer layer ----------------------------------------------------------
@pytest.fixture(params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def size(request):
    return request.param


def fresh(mrt_mod, size, key, cam, frames, precise, moments=False, tmp_factory=None, **kw):
    """(image, moments or None, stats) of a fresh renderer on scene `key` after
    set_camera(cam) (None: the default) and draw(frames)."""
    W0, H0 = size
    ck = ("fresh", size, key, None if cam is None else bytes(cam), frames, precise, moments, tuple(sorted(kw.items())))
    if ck not in _CACHE:
        r = mrt_mod.Renderer(scene(mrt_mod, key, tmp_factory), W0, H0, L0, precise=precise, moments=moments, **kw)
        if cam is not None:
            r.set_camera(cam)
        r.draw(frames)
        _CACHE[ck] = (r.read_image(), r.read_moments() if moments else None, r.stats())
        r.close()
    return _CACHE[ck]


class Stage:
    """The stage calls on device buffers of the renderer tests' size."""

    def __init__(self, mrt_mod, precise, size):
        self.m, self.precise, (self.W, self.H) = mrt_mod, precise, size

    def guides(self, sc, cam=None):
        return guide_planes(self.m, sc, self.W, self.H, cam, self.precise)

    def guides_motion(self, sc, prev, cam=None):
        t = motion_planes(self.m, sc, prev, self.W, self.H, cam, self.precise)
        return (t[0], t[1]), (t[2], t[3])

    def resolve(self, img, frames, hist=None, extra=None):
        d_img, out = to_dev(img), buf(self.W, self.H)
        self.m.temporal_resolve(dev_ptr(d_img), frames, dev_ptr(hist) if hist is not None else None, dev_ptr(out), self.W, self.H)
        if extra is not None:
            d_extra = to_dev(extra)
            self.m.counted_merge(dev_ptr(out), dev_ptr(d_extra), dev_ptr(out), self.W, self.H, precise=self.precise)
        return out

    def reproject(self, prev, g_prev, cam_prev, g_cur):
        out = buf(self.W, self.H)
        self.m.reproject(dev_ptr(prev), dev_ptr(g_prev[0]), dev_ptr(g_prev[1]), cam_prev, dev_ptr(g_cur[0]),
                         dev_ptr(g_cur[1]), dev_ptr(out), self.W, self.H, self.m.ReprojectParams.default())
        return out

    def denoise_variance(self, resolved, moments, g, params):
        var, out, scr = buf(self.W, self.H, c=1), buf(self.W, self.H), buf(self.W, self.H)
        self.m.variance(dev_ptr(moments), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(var), self.W, self.H, params)
        self.m.denoise_variance(dev_ptr(resolved), dev_ptr(var), dev_ptr(g[0]), dev_ptr(g[1]), dev_ptr(out), dev_ptr(scr),
                                None, self.W, self.H, params)
        return host(var, self.W, self.H, 1)[..., 0], host(out, self.W, self.H)


@pytest.mark.parametrize("precise", [True, False])
def test_set_scene_equals_a_fresh_renderer(gpu, mrt_mod, tmp_path_factory, precise, size):
    W0, H0 = size
    A, B, D = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory), camera(mrt_mod, "D")
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise, moments=True)
    r.draw(2)
    r.denoise_variance()
    r.set_scene(B)
    assert r.scene is B and r.stats()["frame_index"] == 0
    # nothing derived survives: no denoised or resolved buffer, no history
    assert status_of(mrt_mod, r.read_denoised) == ERR_STATE and status_of(mrt_mod, r.read_resolved) == ERR_STATE
    assert status_of(mrt_mod, r.read_variance) == ERR_STATE and status_of(mrt_mod, r.resolve) == ERR_STATE
    r.draw(3)
    img, mom, stats = fresh(mrt_mod, size, "B", None, 3, precise, True, tmp_path_factory)
    assert r.read_image().tobytes() == img.tobytes() and r.read_moments().tobytes() == mom.tobytes()
    s = r.stats()
    assert (s["kernel"], s["frame_index"], s["paths"], s["draws"]) == (stats["kernel"], 3, stats["paths"], 1)
    assert s["active_ray_bounces"] == stats["active_ray_bounces"]
    r.resolve()
    res = r.read_resolved()
    assert res[..., :3].tobytes() == img[..., :3].tobytes() and (res[..., 3] == 3.0).all()
    # with a moved camera, which persists across the swap; the draws after it go on from its frames
    r.set_camera(D)
    r.draw(1)
    r.set_scene(A)
    assert r.camera.as_dict() == D.as_dict()
    r.draw(3)
    img, mom, _ = fresh(mrt_mod, size, "A", D, 3, precise, True)
    assert r.read_image().tobytes() == img.tobytes() and r.read_moments().tobytes() == mom.tobytes()
    r.draw(2)
    assert r.read_image().tobytes() == fresh(mrt_mod, size, "A", D, 5, precise, True)[0].tobytes()
    assert status_of(mrt_mod, r.set_scene, mrt_mod.Scene("cornellbox", device=-1)) == ERR_INVALID
    assert r.read_image().tobytes() == fresh(mrt_mod, size, "A", D, 5, precise, True)[0].tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_set_scene_across_kernel_kinds(gpu, mrt_mod, precise, size):
    W0, H0 = size
    """cornellbox to pair (b)'s scene: the kernel is planned again, and the
    renderer launches what a fresh one on that scene launches."""
    A, P = scene(mrt_mod, "A"), scene(mrt_mod, ("P", 512, 1))
    cam = camera(mrt_mod, "A")
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise)
    r.set_camera(cam)
    r.draw(2)
    kind_a = r.stats()["kernel"]
    r.set_scene(P)
    r.draw(3)
    img, _, stats = fresh(mrt_mod, size, ("P", 512, 1), cam, 3, precise)
    assert r.read_image().tobytes() == img.tobytes()
    assert r.stats()["kernel"] == stats["kernel"]
    print(f"kernel kind on cornellbox {kind_a}, on cornellbox + 512 triangles {stats['kernel']}")
    assert stats["kernel"] != kind_a
    r.set_scene(A)          # and back
    r.draw(2)
    assert r.read_image().tobytes() == fresh(mrt_mod, size, "A", cam, 2, precise)[0].tobytes()
    assert r.stats()["kernel"] == kind_a
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_scene_equals_the_stage_replay(gpu, mrt_mod, tmp_path_factory, precise, size):
    W0, H0 = size
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    st = Stage(mrt_mod, precise, size)
    p = mrt_mod.SvgfParams.default()
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise, moments=True)
    r.draw(4)
    img4, mom4 = r.read_image(), r.read_moments()
    r.move_scene(B)
    r.draw(2)               # enqueued behind the move, no sync in between
    r.resolve()
    got, img2, mom2 = r.read_resolved(), r.read_image(), r.read_moments()
    want_img, want_mom, _ = fresh(mrt_mod, size, "B", None, 2, precise, True, tmp_path_factory)
    assert img2.tobytes() == want_img.tobytes() and mom2.tobytes() == want_mom.tobytes()
    gA = st.guides(A)
    gB, motion = st.guides_motion(B, A)
    hist = st.reproject(st.resolve(img4, 4), gA, None, motion)
    mhist = st.reproject(st.resolve(mom4, 4), gA, None, motion)
    res, mres = st.resolve(img2, 2, hist), st.resolve(mom2, 2, mhist)
    assert got.tobytes() == host(res, W0, H0).tobytes()
    assert np.isfinite(got).all() and abs(got[..., 3].max() - 6.0) < 1e-4 and np.mean(got[..., 3] > 2) > 0.5
    # the history follows the block: the pixels that show it now carry more than the two new frames
    moved = (host(motion[1], W0, H0)[..., :3] != host(gB[1], W0, H0)[..., :3]).any(-1)
    assert moved.sum() > 50 and np.mean(got[..., 3][moved] > 2) >= 0.9
    static = host(st.resolve(img2, 2, st.reproject(st.resolve(img4, 4), gA, None, gB)), W0, H0)
    assert np.mean(static[..., 3][moved] > 2) < np.mean(got[..., 3][moved] > 2)
    r.denoise_variance()
    want_var, want = st.denoise_variance(res, mres, gB, p)
    assert r.read_variance().tobytes() == want_var.tobytes() and r.read_denoised().tobytes() == want.tobytes()
    assert r.read_moments().tobytes() == mom2.tobytes() and r.read_image().tobytes() == img2.tobytes()
    # a chain back to A with a camera, through the history just made
    D = camera(mrt_mod, "D")
    r.move_scene(A, D)
    assert r.camera.as_dict() == D.as_dict() and r.scene is A
    r.draw(3)
    r.resolve()
    img3 = r.read_image()
    assert img3.tobytes() == fresh(mrt_mod, size, "A", D, 3, precise, True)[0].tobytes()
    _, motion_back = st.guides_motion(A, B, D)
    want2 = st.resolve(img3, 3, st.reproject(res, gB, None, motion_back))
    assert r.read_resolved().tobytes() == host(want2, W0, H0).tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_scene_to_the_same_geometry_is_move_camera(gpu, mrt_mod, precise, size):
    W0, H0 = size
    A, A2, C = scene(mrt_mod, "A"), scene(mrt_mod, "A2"), camera(mrt_mod, "A")
    out = []
    for move in (lambda r: r.move_scene(A2, C), lambda r: r.move_camera(C)):
        r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise, moments=True)
        r.draw(4)
        move(r)
        r.resolve()
        first = r.read_resolved()           # the pure reprojection
        r.draw(2)
        r.denoise_variance()
        out.append((first, r.read_resolved(), r.read_image(), r.read_moments(), r.read_variance(), r.read_denoised()))
        r.close()
    for a, b in zip(out[0][1:], out[1][1:]):
        assert a.tobytes() == b.tobytes()
    # before the first draw the two differ only where nothing was carried: there the resolve shows the image, which a
    # scene swap clears and a camera move leaves as it was
    carried = out[0][0][..., 3] > 0
    assert np.array_equal(carried, out[1][0][..., 3] > 0) and np.mean(carried) > 0.3
    assert out[0][0][carried].tobytes() == out[1][0][carried].tobytes() and not out[0][0][~carried].any()
    # on a fresh renderer there is nothing to carry: set_scene plus set_camera
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise)
    r.move_scene(A2, C)
    assert status_of(mrt_mod, r.resolve) == ERR_STATE and r.camera.as_dict() == C.as_dict()
    r.draw(2)
    assert r.read_image().tobytes() == fresh(mrt_mod, size, "A", C, 2, precise)[0].tobytes()
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_scene_carries_and_clears_the_extra_images(gpu, mrt_mod, tmp_path_factory, precise, size):
    W0, H0 = size
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    st = Stage(mrt_mod, precise, size)
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=precise, moments=True)
    r.draw(3)
    r.draw_tiles([0], 2)
    img3, mom3, E, EM = r.read_image(), r.read_moments(), r.read_extra(), r.read_extra_moments()
    assert (E[..., 3] == 2).all() and (EM[..., 3] == 2).all()      # one tile covers the 64x48 frame
    r.move_scene(B)
    assert not r.read_extra().any() and not r.read_extra_moments().any()
    r.resolve()
    gA = st.guides(A)
    _, motion = st.guides_motion(B, A)
    hist = st.reproject(st.resolve(img3, 3, extra=E), gA, None, motion)
    zero = np.zeros((H0, W0, 4), np.float32)
    got = r.read_resolved()
    assert got.tobytes() == host(st.resolve(zero, 0, hist), W0, H0).tobytes()
    assert abs(got[..., 3].max() - 5.0) < 1e-4
    # ... and EM into the moments history: the variance plane and the filtered image of the pure reprojection
    mhist = st.reproject(st.resolve(mom3, 3, extra=EM), gA, None, motion)
    gB = st.guides(B)
    r.denoise_variance()
    want_var, want = st.denoise_variance(st.resolve(zero, 0, hist), st.resolve(zero, 0, mhist), gB,
                                         mrt_mod.SvgfParams.default())
    assert r.read_variance().tobytes() == want_var.tobytes() and r.read_denoised().tobytes() == want.tobytes()
    unmerged = st.denoise_variance(st.resolve(zero, 0, hist), st.resolve(zero, 0, st.reproject(st.resolve(mom3, 3), gA, None, motion)),
                                   gB, mrt_mod.SvgfParams.default())
    assert unmerged[0].tobytes() != want_var.tobytes()       # the comparison does see EM
    r.draw_tiles([0], 1)        # the extras go on from zero, the refine schedule from where it was
    assert (r.read_extra()[..., 3] == 1).all() and r.refine_stats()["extra_frames"] == 3
    r.close()


@pytest.mark.parametrize("precise", [True, False])
def test_move_scene_errors_change_nothing(gpu, mrt_mod, tmp_path_factory, precise, size):
    W0, H0 = size
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    P = scene(mrt_mod, ("P", 512, 1))
    r, twin = (mrt_mod.Renderer(A, W0, H0, L0, precise=precise) for _ in range(2))
    for x in (r, twin):
        x.draw(2)
    with pytest.raises(mrt_mod.MrtError, match="triangles") as e:
        r.move_scene(P)                                        # an incompatible scene
    assert e.value.status == ERR_INVALID
    bad = mrt_mod.Camera.default()
    bad.tan_half_fov = 0.0
    assert status_of(mrt_mod, r.move_scene, B, bad) == ERR_INVALID
    with pytest.raises(mrt_mod.MrtError, match="plane_tolerance"):
        r.move_scene(B, None, mrt_mod.ReprojectParams(-1.0, 0.9, 32.0))
    assert status_of(mrt_mod, r.move_scene, mrt_mod.Scene("cornellbox", device=-1)) == ERR_INVALID
    assert r.scene is A and r.stats()["frame_index"] == 2
    for x in (r, twin):                                        # it goes on as one that never made the calls
        x.draw(2)
        x.move_camera(camera(mrt_mod, "D"))
        x.draw(1)
        x.resolve()
    assert r.read_image().tobytes() == twin.read_image().tobytes()
    assert r.read_resolved().tobytes() == twin.read_resolved().tobytes()
    r.close()
    twin.close()


def test_set_scene_clears_an_external_image_and_drops_a_pending_exchange(gpu, mrt_mod, tmp_path_factory, size):
    W0, H0 = size
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    want = fresh(mrt_mod, size, "B", None, 2, True, False, tmp_path_factory)[0]
    # an external image: resize refuses it, set_scene clears it as reset does
    d_img = buf(W0, H0, 3.0)
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=True, image_ptr=dev_ptr(d_img))
    r.draw(2)
    r.set_scene(B)
    r.sync()
    assert r.image_ptr() == dev_ptr(d_img) and not host(d_img, W0, H0).any()
    r.draw(2)
    assert r.read_image().tobytes() == want.tobytes() and host(d_img, W0, H0).tobytes() == want.tobytes()
    r.close()
    # a deferred (overlapped) gather of the old scene's tiles is dropped, never unpacked into the new image
    comm = mrt_mod.Comm(mrt_mod.comm_unique_id(), 1, 0, 0)
    r = mrt_mod.Renderer(A, W0, H0, L0, precise=True)
    r.draw(3)
    r.exchange(comm, mrt_mod.EXCHANGE_GATHER | mrt_mod.EXCHANGE_OVERLAP)
    r.set_scene(B)
    r.draw(2)
    assert r.read_image().tobytes() == want.tobytes()
    # and a scene the call refuses leaves the pending gather to land as it would have
    r.exchange(comm, mrt_mod.EXCHANGE_GATHER | mrt_mod.EXCHANGE_OVERLAP)
    assert status_of(mrt_mod, r.set_scene, mrt_mod.Scene("cornellbox", device=-1)) == ERR_INVALID
    assert r.read_image().tobytes() == want.tobytes()
    r.close()
    comm.close()


@pytest.mark.parametrize("precise", [True, False])
def test_sharded_renderer(gpu, mrt_mod, tmp_path_factory, precise):
    """A sharded renderer keeps no history: move_scene is MRT_ERR_STATE; set_scene works."""
    A, B = scene(mrt_mod, "A"), scene(mrt_mod, "B", tmp_path_factory)
    W, H = 160, 96          # 3 x 2 tiles: rank 1 of 2 owns three of them
    r = mrt_mod.Renderer(A, W, H, L0, precise=precise, shard_rank=1, shard_count=2)
    r.draw(2)
    assert status_of(mrt_mod, r.move_scene, B) == ERR_STATE
    assert r.scene is A and r.stats()["frame_index"] == 2
    r.set_scene(B)
    r.draw(2)
    f = mrt_mod.Renderer(B, W, H, L0, precise=precise, shard_rank=1, shard_count=2)
    f.draw(2)
    got = r.read_image()
    assert got.tobytes() == f.read_image().tobytes() and got.any() and not got[:64, :64].any()
    assert r.stats()["owned_pixels"] == f.stats()["owned_pixels"]
    r.close()
    f.close()


@pytest.mark.parametrize("precise", [True, False])
def test_cli_then_scene(gpu, mrt_mod, tmp_path, precise, size):
    W0, H0 = size
    """mrt_render --then-scene writes the resolved image (or with
    --denoise-variance the filtered one) of the same sequence through the binding."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    obj2 = moved_obj(mrt_mod, tmp_path)
    base = [exe, "--scene", "cornellbox", "--w", str(W0), "--h", str(H0), "--spp", "2", "--L", "4", "--then-scene", obj2,
            "--then-mtl", mtl_path(mrt_mod)] + (["--precise"] if precise else [])

    def run(extra, name):
        out = tmp_path / name
        p = subprocess.run(base + extra + ["--out", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        with open(out, "rb") as f:
            assert f.readline().strip() == b"PF"
            w, h = map(int, f.readline().split())
            assert (w, h) == (W0, H0) and float(f.readline()) < 0
            return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)

    B = mrt_mod.Scene(obj2, mtl_path(mrt_mod))
    for moments, extra, name in ((False, [], "a.pfm"), (True, ["--denoise-variance"], "b.pfm")):
        r = mrt_mod.Renderer(scene(mrt_mod, "A"), W0, H0, 4, precise=precise, moments=moments)
        r.draw(2)
        r.move_scene(B)
        r.draw(2)
        if moments:
            r.denoise_variance()
            want = r.read_denoised()
        else:
            r.resolve()
            want = r.read_resolved()
            assert abs(want[..., 3].max() - 4.0) < 1e-4
        assert run(extra, name).tobytes() == np.ascontiguousarray(want[..., :3]).tobytes()
        r.close()
    p = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "single rank" in p.stderr
    p = subprocess.run([exe, "--then-mtl", "x.mtl"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--then-scene" in p.stderr
    p = subprocess.run(base + ["--scene", "CornellBox-Water", "--out", str(tmp_path / "c.pfm")],   # (the last --scene counts)
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "mrt_renderer_move_scene" in p.stderr and "triangles" in p.stderr
