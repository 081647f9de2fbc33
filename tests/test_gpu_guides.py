"""mrt_guides against the stage pipeline it restates: mrt.raygen on a
constant-0.5 noise table (the pixel-centre ray; the ray buffer is zeroed, so
tmin = 0) and mrt.intersect, both pinned bitwise elsewhere
(test_gpu_parity.py, test_gpu_camera.py), turned into the expected planes by
tests/denoise_model.py guides_from_hits."""
import numpy as np
import pytest

from camera_cases import camera
from denoise_model import MISS_WORD, NOT_FILTERABLE, guides_from_hits, words
from helpers import dev_ptr, from_dev, to_dev

pytestmark = pytest.mark.gpu

CENTRE = np.full(64 * 64 * 4, 0.5, np.float32)


def _scene(mrt_mod, key, cache={}):
    if key not in cache:
        name, procedural = key
        # device PLOC builds the deepest trees: 1M triangles need 75 stack entries (400 K: 66; LBVH 1M: 62)
        cache[key] = mrt_mod.Scene(name, procedural_triangles=procedural,
                                   bvh_builder=mrt_mod.BVH_DEVICE_PLOC if procedural else 0)
    return cache[key]


def _planes(mrt_mod, sc, W, H, cam=None, precise=True):
    d_n, d_p = to_dev(np.zeros(W * H * 4, np.float32)), to_dev(np.zeros(W * H * 4, np.float32))
    mrt_mod.guides(sc, W, H, dev_ptr(d_n), dev_ptr(d_p), camera=cam, precise=precise)
    return from_dev(d_n, np.float32).reshape(-1, 4), from_dev(d_p, np.float32).reshape(-1, 4)


def _stage_hits(mrt_mod, oracle_mod, sc, W, H, cam=None, precise=True):
    d_rays = to_dev(np.zeros(W * H, oracle_mod.RAY_DTYPE))
    mrt_mod.raygen(sc, W, H, dev_ptr(to_dev(CENTRE)), dev_ptr(d_rays), precise=precise, camera=cam)
    d_isect = to_dev(np.zeros(W * H, oracle_mod.ISECT_DTYPE))
    mrt_mod.intersect(sc, dev_ptr(d_rays), 80, W * H, dev_ptr(d_isect), precise=precise)
    return from_dev(d_rays, oracle_mod.RAY_DTYPE), from_dev(d_isect, oracle_mod.ISECT_DTYPE)


def _pinhole(mrt_mod, name):
    return None if name is None else camera(mrt_mod, name)


CASES = [
    (("cornellbox", 0), 64, 48, None),
    (("cornellbox", 0), 37, 29, None),               # no tile or block size divides it
    (("CornellBox-Water", 0), 64, 48, None),         # several materials, light hits and misses
    (("cornellbox", 0), 64, 48, "A"),                # a moved pinhole camera
    (("cornellbox", 0), 32, 32, "B"),                # from outside: misses
    (("cornellbox", 1 << 20), 32, 32, None),         # deep tree: the spill variant of the traversal stack
    (("cornellbox", 1 << 20), 640, 480, None),       # ... with 1200 blocks of pixels: more than its persistent grid of
                                                     # 1024, so its last blocks' spill rows and its grid-stride loop
]


@pytest.mark.parametrize("key,W,H,cam_name", CASES)
def test_guides_precise_bitwise(gpu, mrt_mod, oracle_mod, key, W, H, cam_name):
    sc, cam = _scene(mrt_mod, key), _pinhole(mrt_mod, cam_name)
    if key[1]:
        assert sc.info["bvh_max_stack"] > 64, sc.info["bvh_max_stack"]   # the case is about the spill variant
    rays, isect = _stage_hits(mrt_mod, oracle_mod, sc, W, H, cam)
    want_n, want_p = guides_from_hits(sc.export(), isect, rays)
    got_n, got_p = _planes(mrt_mod, sc, W, H, cam)
    w = words(want_n)
    print(f"{key} {W}x{H} camera {cam_name}: filterable {np.mean(w < NOT_FILTERABLE):.3f}, "
          f"lights {np.mean((w >= NOT_FILTERABLE) & (w != MISS_WORD)):.3f}, misses {np.mean(w == MISS_WORD):.3f}, "
          f"materials {len(np.unique(w[w < NOT_FILTERABLE]))}")
    assert (w < NOT_FILTERABLE).any()
    assert np.array_equal(words(got_n), w)
    assert got_p.tobytes() == want_p.tobytes()                       # x and t
    assert got_n[:, :3].tobytes() == want_n[:, :3].tobytes()         # n
    # misses: n = 0, x = 0, t = -1
    miss = w == MISS_WORD
    assert np.all(got_n[miss, :3] == 0) and np.all(got_p[miss, :3] == 0) and np.all(got_p[miss, 3] == -1.0)


def test_scene_mix(gpu, mrt_mod):
    """The cases above do cover what they claim: the water scene shows several
    materials and a light, the outside camera misses."""
    gn, _ = _planes(mrt_mod, _scene(mrt_mod, ("CornellBox-Water", 0)), 64, 48)
    w = words(gn)
    assert len(np.unique(w[w < NOT_FILTERABLE])) >= 3
    assert ((w >= NOT_FILTERABLE) & (w != MISS_WORD)).any()
    gn, _ = _planes(mrt_mod, _scene(mrt_mod, ("cornellbox", 0)), 32, 32, camera(mrt_mod, "B"))
    assert (words(gn) == MISS_WORD).any()


def test_lens_is_ignored(gpu, mrt_mod):
    """Camera E is camera A with a thin lens: the guide ray goes through the pinhole."""
    sc = _scene(mrt_mod, ("cornellbox", 0))
    a_n, a_p = _planes(mrt_mod, sc, 64, 48, camera(mrt_mod, "A"))
    e_n, e_p = _planes(mrt_mod, sc, 64, 48, camera(mrt_mod, "E"))
    assert camera(mrt_mod, "E").lens_radius > 0
    assert a_n.tobytes() == e_n.tobytes() and a_p.tobytes() == e_p.tobytes()
    # the default pose with a lens is the default camera
    d = mrt_mod.Camera.default()
    d.lens_radius, d.focus_distance = 0.1, 2.0
    d_n, d_p = _planes(mrt_mod, sc, 64, 48, d)
    n_n, n_p = _planes(mrt_mod, sc, 64, 48, None)
    assert d_n.tobytes() == n_n.tobytes() and d_p.tobytes() == n_p.tobytes()


def test_bad_arguments(gpu, mrt_mod):
    sc = _scene(mrt_mod, ("cornellbox", 0))
    buf = to_dev(np.zeros(64 * 48 * 4, np.float32))
    other = to_dev(np.zeros(64 * 48 * 4, np.float32))
    for args in [(1, 48, dev_ptr(buf), dev_ptr(other)), (64, 48, None, dev_ptr(other)),
                 (64, 48, dev_ptr(buf), dev_ptr(buf))]:
        with pytest.raises(mrt_mod.MrtError) as e:
            mrt_mod.guides(sc, *args)
        assert e.value.status == -1
    bad = mrt_mod.Camera.default()
    bad.tan_half_fov = -1.0
    with pytest.raises(mrt_mod.MrtError, match="tan_half_fov"):
        mrt_mod.guides(sc, 64, 48, dev_ptr(buf), dev_ptr(other), camera=bad)


@pytest.mark.parametrize("key", [("cornellbox", 0), ("CornellBox-Water", 0)])
def test_guides_fast_build(gpu, mrt_mod, oracle_mod, key):
    """Fast build: word equal and t within 1e-4 relative of the oracle's planes
    on at least the share of pixels on which the fast stage pipeline (raygen +
    intersect, the subject of test_intersect_matches_bruteforce's fast gate:
    same hit state and primitive, t to 1e-4) agrees with the oracle on the same
    scene and rays.  Measured on an MI355X at 64x48: cornellbox both shares
    1.00000, CornellBox-Water both 1.00000."""
    W, H = 64, 48
    sc = _scene(mrt_mod, key)
    osc = oracle_mod.OracleScene(mrt_mod.scene_path(key[0]))
    rays = oracle_mod.raygen(W, H, CENTRE)
    ref = osc.intersect(rays)
    want_n, want_p = guides_from_hits(osc, ref, rays)
    _, got = _stage_hits(mrt_mod, oracle_mod, sc, W, H, None, precise=False)
    hit_ref, hit_got = ref["distance"] >= 0, got["distance"] >= 0
    close = np.abs(got["distance"] - ref["distance"]) <= 1e-4 * np.abs(ref["distance"])
    gate = (hit_ref == hit_got) & (~hit_ref | ((got["triangleIndex"] == ref["triangleIndex"]) & close))
    got_n, got_p = _planes(mrt_mod, sc, W, H, None, precise=False)
    share = (words(got_n) == words(want_n)) & (np.abs(got_p[:, 3] - want_p[:, 3]) <= 1e-4 * np.abs(want_p[:, 3]))
    err_x = np.abs(got_p[share, :3] - want_p[share, :3]).max()
    err_n = np.abs(got_n[share, :3] - want_n[share, :3]).max()
    print(f"fast guides {key[0]}: share {share.mean():.5f}, stage pipeline's share {gate.mean():.5f}, "
          f"max |x| error {err_x:.3g}, max |n| error {err_n:.3g}")
    assert share.mean() >= gate.mean()
    assert np.isfinite(got_n[:, :3]).all() and np.isfinite(got_p).all()


def test_renderer_guide_pass_on_a_deep_scene(gpu, mrt_mod):
    """mrt_renderer_denoise on the deep scene at 640x480 (the spill variant over
    its whole persistent grid, with the renderer's own spill buffer) equals the
    stage pipeline, and a second renderer denoising the same scene on its own
    stream at the same time changes nothing."""
    W, H, L = 640, 480, 4
    sc = _scene(mrt_mod, ("cornellbox", 1 << 20))
    r, other = (mrt_mod.Renderer(sc, W, H, L, precise=True) for _ in range(2))
    r.draw(1)
    other.draw(1)
    r.denoise()        # both enqueued before either is waited for
    other.denoise()
    got, img = r.read_denoised(), r.read_image()
    assert other.read_denoised().tobytes() == got.tobytes()
    d_img = to_dev(img)
    d_n, d_p, d_out, d_scr = (to_dev(np.zeros((H, W, 4), np.float32)) for _ in range(4))
    mrt_mod.guides(sc, W, H, dev_ptr(d_n), dev_ptr(d_p), precise=True)
    mrt_mod.denoise(dev_ptr(d_img), dev_ptr(d_n), dev_ptr(d_p), dev_ptr(d_out), dev_ptr(d_scr), W, H,
                    mrt_mod.DenoiseParams.default(1))
    assert got.tobytes() == from_dev(d_out, np.float32).tobytes()
    assert np.abs(got - img).max() > 1e-3
    r.close()
    other.close()
