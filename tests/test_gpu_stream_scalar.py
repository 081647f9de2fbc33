"""GPU: the stream kernel with the scalar side of its hot loops cut back
 changes no pixel — phase 1 of the nearest sweep reads the centre
list in groups of four records and the rest one by one, with one exec save for
both loops and the id from the record; the sweep's
and the camera lists' leaf tests use the short acceptance predicates of
tri_accept.h and h.found is derived from h.prim.  Fresh scene and renderer per
render, 2 frames, both builds:

a. the sweep is bitwise equal, image and active-ray count, to MRT_SWEEP=0 (the
   walk, which keeps the full predicates and has no phase 1);
b. the stream kernel is bitwise equal to the per-bounce kernels (MRT_STREAM=0);
c. the precise build is bit-identical to the oracle, active rays included.

Shapes: 64 x 48 and a ragged 97 x 61, L = 1 ... 5, the Cornell box (18
records: four groups and two single records) and generated rooms of 12 (whole
groups), 18, 30 (next to the cap of 32) and 17 records (wedge: one single
record).  roomgen's rooms come to 12,
16, 17, 18, 24, 25 or 30 records — six per block and six for the room, five
for a block without a bottom or a wedge, seven more for a second light — and
a fifth block leaves the sweep, so there is no 32-record room.  Once each a
moved camera (the CAM = true instantiation, origins inside record boxes) and
the tile list (the LIST = true instantiation: draw_tiles over every tile is a
draw with the refine seed).  Milliseconds per render, under a second per
oracle render."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 2
SCENES = {"cornellbox": 18, "plain-1": 12, "stacked": 18, "plain-4": 30, "wedge": 17}
UNROLL = 4   # dev_sweep.h kSweepUnroll


@pytest.fixture(scope="module")
def scene(mrt_mod, tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_stream_scalar"), {}

    def get(name):
        if name not in cache:
            cache[name] = (mrt_mod.scene_path(name) if name == "cornellbox"
                           else roomgen.room(name, roomgen.seeds(name)[0], d).path)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(image, active rays) of the oracle, rendered once per (scene, size, L, seed)."""
    cache = {}

    def get(path, size, L, seed=SEED):
        key = (path, size, L, seed)
        if key not in cache:
            cache[key] = oracle_mod.OracleScene(path).render(size[0], size[1], L, seed, FRAMES, threads=8)
            assert np.isfinite(cache[key][0]).all() and cache[key][0][..., :3].max() > 0
        return cache[key]
    return get


def _render(mrt_mod, monkeypatch, path, size, L, precise, sweep=True, stream=True, cam=None, tiles=False, seed=SEED):
    """(image, active ray bounces, sweep enabled, phase-1 entries) of a fresh scene and renderer;
    tiles: the extra image of draw_tiles over every tile instead of the image of draw."""
    monkeypatch.setenv("MRT_SWEEP", "1" if sweep else "0")
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    s = mrt_mod.Scene(path)
    enabled, entries = mrt_mod.debug_sweep_list(s)[0], len(mrt_mod.debug_sweep_phase1(s))
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
    return img, active, enabled, entries


def _check(mrt_mod, monkeypatch, path, size, L, records, what, ref=None, cam=None):
    for precise in (True, False):
        build = "precise" if precise else "fast"
        a, na, on, entries = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam)
        assert on and entries == records and np.isfinite(a).all() and a[..., :3].max() > 0
        for other, kw in (("walk", dict(sweep=False)), ("per-bounce kernels", dict(stream=False))):
            b, nb, on_b, entries_b = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam, **kw)
            assert on_b == (other != "walk") and entries_b == (records if on_b else 0)
            same = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
            print(f"{what} {build}: sweep vs {other}: bit-identical {same:.5f}, rays {na} / {nb}")
            assert a.tobytes() == b.tobytes() and na == nb
        if precise and ref is not None:
            rel, rmse, same = pixel_metrics(a, ref[0])
            print(f"{what} precise vs oracle: bit-identical {same:.5f}, rmse {rmse:.2e}, rays {na} vs {ref[1]}")
            assert same == 1.0 and na == ref[1]


def test_the_rooms_cover_whole_and_broken_groups():
    counts = sorted(set(SCENES.values()))
    assert any(n % UNROLL == 0 for n in counts) and {n % UNROLL for n in counts} >= {0, 1, 2}
    assert max(counts) + UNROLL > 32   # the mask's high bits


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
@pytest.mark.parametrize("name", list(SCENES))
def test_sweep_equals_walk_per_bounce_and_oracle(gpu, mrt_mod, monkeypatch, scene, reference, name, size, L):
    path = scene(name)
    _check(mrt_mod, monkeypatch, path, size, L, SCENES[name], f"{name} {size[0]}x{size[1]} L={L}",
           ref=reference(path, size, L))


@pytest.mark.parametrize("name", ["plain-4", "wedge"])
def test_moved_camera_inside_the_room(gpu, mrt_mod, monkeypatch, scene, name):
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    _check(mrt_mod, monkeypatch, scene(name), (97, 61), 5, SCENES[name], f"{name}, moved camera", cam=cam)


@pytest.mark.parametrize("name", ["cornellbox", "plain-4", "wedge"])
def test_tile_list_instantiation(gpu, mrt_mod, monkeypatch, scene, reference, name):
    """draw_tiles over every tile (the LIST = true stream kernel): its extra
    image is bitwise the walk's in both builds, and the image of a plain draw
    with the refine seed by the per-bounce kernels; the precise build's is the
    oracle's with that seed."""
    path, size, L = scene(name), (97, 61), 4
    seed = SEED ^ mrt_mod.REFINE_SEED_XOR
    for precise in (True, False):
        a = _render(mrt_mod, monkeypatch, path, size, L, precise, tiles=True)[0]
        b = _render(mrt_mod, monkeypatch, path, size, L, precise, tiles=True, sweep=False)[0]
        c, nc, _, _ = _render(mrt_mod, monkeypatch, path, size, L, precise, stream=False, seed=seed)
        assert a.tobytes() == b.tobytes()
        assert a[..., :3].tobytes() == c[..., :3].tobytes()
        if precise:
            ref = reference(path, size, L, seed)
            rel, rmse, same = pixel_metrics(c, ref[0])
            print(f"{name} tile list, precise vs oracle: bit-identical {same:.5f}, rays {nc} vs {ref[1]}")
            assert same == 1.0 and nc == ref[1]
