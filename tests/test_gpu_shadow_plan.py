"""GPU: the shadow query with one entry-face pass for all convex solids
(dev_shadow.h convex_occlusion, shadow_plan.h) changes no pixel.
Fresh scene and renderer per render, 2 frames:

a. precise build: bit-identical to the oracle with equal active-ray counts, and
   bitwise equal to the convex test off (MRT_CONVEX=0: the occluder tree walked);
b. fast build: the stream kernel bitwise equal to the per-bounce kernels
   (MRT_STREAM=0), and inside the fast gate against the oracle.

Shapes: 64 x 48 and a ragged 97 x 61, L = 2 ... 5, the Cornell box (2 solids)
and generated rooms: plain-1 (1 solid: no later solid), plain-4 (4 solids: the
plan's whole mask), stacked and crossing (lanes that cross two solids, segments
that start inside a padded solid: no entry face) and wedge (detection fails:
the walk).  Once each a moved camera and the tile list.  Milliseconds per
render, under a second per oracle render."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 2
SCENES = {"cornellbox": 2, "plain-1": 1, "plain-4": 4, "stacked": 2, "crossing": 2, "wedge": 0}   # convex solids


@pytest.fixture(scope="module")
def scene(mrt_mod, tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_shadow_plan"), {}

    def get(name):
        if name not in cache:
            cache[name] = (mrt_mod.scene_path(name) if name == "cornellbox"
                           else roomgen.room(name, roomgen.seeds(name)[0], d).path)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(image, active rays) of the oracle, rendered once per (scene, size, L, seed), never written to."""
    cache = {}

    def get(path, size, L, seed=SEED):
        key = (path, size, L, seed)
        if key not in cache:
            img, A = oracle_mod.OracleScene(path).render(size[0], size[1], L, seed, FRAMES, threads=8)
            assert np.isfinite(img).all() and img[..., :3].max() > 0
            img.setflags(write=False)
            cache[key] = (img, A)
        return cache[key]
    return get


def _render(mrt_mod, monkeypatch, path, size, L, precise, convex=True, stream=True, cam=None, tiles=False, seed=SEED):
    """(image, active ray bounces, convex solids detected) of a fresh scene and renderer;
    tiles: the extra image of draw_tiles over every tile instead of the image of draw."""
    monkeypatch.setenv("MRT_CONVEX", "1" if convex else "0")
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    s = mrt_mod.Scene(path)
    solids = s.info["convex_solids"]
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise, moments=tiles, seed=seed)
    if cam is not None:
        r.set_camera(cam)
    assert r.stats()["kernel"] == (2 if stream else 0)
    if tiles:
        r.draw_tiles(np.arange(r.tile_count())[::-1], FRAMES)
        img, active = r.read_extra(), None
        assert (img[..., 3] == FRAMES).all()
    else:
        r.draw(FRAMES)
        img, st = r.read_image(), r.stats()
        active = st["active_ray_bounces"]
        assert st["paths"] == size[0] * size[1] * FRAMES
    r.close()
    s.close()
    return img, active, solids


def _fast_gate(a, ref, what):
    """test_gpu_rooms' fast gate against the oracle; the bit-identical share is printed."""
    rel, rmse, same = pixel_metrics(a, ref)
    print(f"{what} fast vs oracle: bit-identical {same:.5f}, rel<=1e-2 {np.mean(rel <= 1e-2):.5f}, rmse {rmse:.2e}")
    assert np.mean(rel <= 1e-2) >= 0.99


def _check(mrt_mod, monkeypatch, path, size, L, solids, what, ref, cam=None):
    a, na, found = _render(mrt_mod, monkeypatch, path, size, L, True, cam=cam)
    assert found == solids and np.isfinite(a).all() and a[..., :3].max() > 0
    b, nb, off = _render(mrt_mod, monkeypatch, path, size, L, True, convex=False, cam=cam)
    assert off == 0
    rel, rmse, same = pixel_metrics(a, ref[0])
    print(f"{what} precise: vs oracle bit-identical {same:.5f}, rays {na} vs {ref[1]}; "
          f"vs convex off {(a.view(np.uint32) == b.view(np.uint32)).all(-1).mean():.5f}, rays {nb}")
    assert same == 1.0 and na == ref[1]
    assert a.tobytes() == b.tobytes() and na == nb
    f, nf, found = _render(mrt_mod, monkeypatch, path, size, L, False, cam=cam)
    g, ng, _ = _render(mrt_mod, monkeypatch, path, size, L, False, stream=False, cam=cam)
    print(f"{what} fast: stream vs per-bounce kernels bit-identical "
          f"{(f.view(np.uint32) == g.view(np.uint32)).all(-1).mean():.5f}, rays {nf} / {ng}")
    assert found == solids and f.tobytes() == g.tobytes() and nf == ng
    _fast_gate(f, ref[0], what)


def test_the_scenes_cover_the_plan():
    """One solid (no later solids), the whole mask, two-solid crossings and a scene without the convex test."""
    assert {1, 4, 0} <= set(SCENES.values()) and roomgen.CASES["stacked"][0] == roomgen.CASES["crossing"][0] == 2
    assert all(roomgen.CASES[n][0] == c for n, c in SCENES.items() if n != "cornellbox")


@pytest.mark.parametrize("L", [2, 3, 4, 5])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
@pytest.mark.parametrize("name", list(SCENES))
def test_one_pass_equals_oracle_convex_off_and_per_bounce(gpu, mrt_mod, monkeypatch, scene, reference, name, size, L):
    path = scene(name)
    _check(mrt_mod, monkeypatch, path, size, L, SCENES[name], f"{name} {size[0]}x{size[1]} L={L}",
           reference(path, size, L))


def test_moved_camera_inside_the_room(gpu, mrt_mod, monkeypatch, scene):
    """Camera rays that start between the solids: bounce-0 shadow rays from everywhere in the room.
    (The oracle renders the default camera only: here the precise build stands against convex off.)"""
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    path, size, L = scene("plain-4"), (97, 61), 5
    for precise in (True, False):
        a, na, found = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam)
        assert found == 4 and np.isfinite(a).all() and a[..., :3].max() > 0
        g, ng, _ = _render(mrt_mod, monkeypatch, path, size, L, precise, stream=False, cam=cam)
        assert a.tobytes() == g.tobytes() and na == ng
        if precise:
            b, nb, off = _render(mrt_mod, monkeypatch, path, size, L, True, convex=False, cam=cam)
            assert off == 0 and a.tobytes() == b.tobytes() and na == nb


def test_tile_list_instantiation(gpu, mrt_mod, monkeypatch, scene, reference):
    """draw_tiles over every tile (the LIST = true stream kernel): its extra image is bitwise convex off's in
    the precise build, and the image of a plain draw with the refine seed by the per-bounce kernels in both;
    the precise build's is the oracle's with that seed."""
    path, size, L = scene("crossing"), (97, 61), 4
    seed = SEED ^ mrt_mod.REFINE_SEED_XOR
    for precise in (True, False):
        a = _render(mrt_mod, monkeypatch, path, size, L, precise, tiles=True)[0]
        c, nc, _ = _render(mrt_mod, monkeypatch, path, size, L, precise, stream=False, seed=seed)
        assert a[..., :3].tobytes() == c[..., :3].tobytes()
        if precise:
            b = _render(mrt_mod, monkeypatch, path, size, L, True, tiles=True, convex=False)[0]
            assert a.tobytes() == b.tobytes()
            ref = reference(path, size, L, seed)
            rel, rmse, same = pixel_metrics(c, ref[0])
            print(f"crossing tile list, precise vs oracle: bit-identical {same:.5f}, rays {nc} vs {ref[1]}")
            assert same == 1.0 and nc == ref[1]
