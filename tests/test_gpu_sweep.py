"""GPU: the leaf-box sweep (dev_sweep.h sweep_nearest) returns
the walk's answer for every nearest query — on the Cornell box (64 x 48 and a
ragged 97 x 61, L = 1 ... 5) and on generated rooms (96 x 64, L = 4), 3 frames:

a. the precise build is bit-identical to the oracle, with equal active-ray
   counts;
b. in each build the default (the sweep, where the scene is eligible) is
   bitwise equal to MRT_SWEEP=0 (the walk);
c. the stream and per-bounce kernels are bitwise equal.

One room is over the leaf cap and must take the walk; one eligible room is
rendered through a moved camera (the kernels' CAM = true instantiation).
Milliseconds per render, under a second per oracle render."""
import numpy as np
import pytest

import roomgen
from camera_cases import replay_render
from helpers import SEED, dev_ptr, from_dev, pixel_metrics, to_dev

pytestmark = pytest.mark.gpu

FRAMES = 3
ELIGIBLE = ["plain-1", "plain-4", "stacked", "float"]
INELIGIBLE = "plain-5"


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_sweep"), {}

    def get(name):
        if name not in cache:
            cache[name] = roomgen.room(name, roomgen.seeds(name)[0], d).path
        return cache[name]
    return get


def _render(mrt_mod, monkeypatch, path, size, L, precise, sweep=True, stream=True, cam=None):
    """(image, active ray bounces, sweep enabled) of a fresh scene and renderer."""
    monkeypatch.setenv("MRT_SWEEP", "1" if sweep else "0")
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    s = mrt_mod.Scene(path)
    enabled, _ = mrt_mod.debug_sweep_list(s)
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise)
    if cam is not None:
        r.set_camera(cam)
    r.draw(FRAMES)
    img, st = r.read_image(), r.stats()
    r.close()
    s.close()
    assert st["kernel"] == (2 if stream else 0) and st["paths"] == size[0] * size[1] * FRAMES
    return img, st["active_ray_bounces"], enabled


def _check(mrt_mod, monkeypatch, path, size, L, eligible, ref=None, cam=None, what=""):
    """b. and c. in both builds; a. against `ref` = (image, active rays) when given."""
    for precise in (True, False):
        a, na, on = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam)
        w, nw, off = _render(mrt_mod, monkeypatch, path, size, L, precise, sweep=False, cam=cam)
        b, nb, _ = _render(mrt_mod, monkeypatch, path, size, L, precise, stream=False, cam=cam)
        assert on == eligible and not off
        assert np.isfinite(a).all() and a[..., :3].max() > 0
        same_w = (a.view(np.uint32) == w.view(np.uint32)).all(-1).mean()
        same_b = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
        print(f"{what} {'precise' if precise else 'fast'}: sweep {on}, vs walk bit-identical {same_w:.5f} "
              f"(rays {na} / {nw}), stream vs per-bounce {same_b:.5f} (rays {na} / {nb})")
        assert a.tobytes() == w.tobytes() and na == nw
        assert a.tobytes() == b.tobytes() and na == nb
        if precise and ref is not None:
            rel, rmse, same = pixel_metrics(a, ref[0])
            print(f"{what} precise vs oracle: bit-identical {same:.5f}, rmse {rmse:.2e}, rays {na} vs {ref[1]}")
            assert same == 1.0 and na == ref[1]


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
def test_cornell_box_sweep_equals_walk_and_oracle(gpu, mrt_mod, oracle_mod, monkeypatch, size, L):
    path = mrt_mod.scene_path("cornellbox")
    ref = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
    assert np.isfinite(ref[0]).all() and ref[0][..., :3].max() > 0
    _check(mrt_mod, monkeypatch, path, size, L, True, ref, what=f"cornellbox {size[0]}x{size[1]} L={L}")


@pytest.mark.parametrize("name", ELIGIBLE + [INELIGIBLE])
def test_rooms_sweep_equals_walk_and_oracle(gpu, mrt_mod, oracle_mod, monkeypatch, room, name):
    """The four eligible rooms sweep; plain-5's tree has more than 32 leaves
    and walks (asserted through the scene's own report)."""
    path, size, L = room(name), (96, 64), 4
    ref = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
    assert np.isfinite(ref[0]).all() and ref[0][..., :3].max() > 0
    _check(mrt_mod, monkeypatch, path, size, L, name != INELIGIBLE, ref, what=name)


def test_moved_camera_sweep_equals_walk(gpu, mrt_mod, oracle_mod, monkeypatch, room):
    """An eligible room through a camera inside it (CAM = true kernels): b. and
    c., and the precise build against the oracle's stages replayed from the
    GPU's own camera rays (test_gpu_rooms' moved-camera gate)."""
    path, size, L = room("stacked"), (97, 61), 4
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    _check(mrt_mod, monkeypatch, path, size, L, True, cam=cam, what="stacked, moved camera")
    a, _, on = _render(mrt_mod, monkeypatch, path, size, L, True, cam=cam)
    assert on
    sc, osc = mrt_mod.Scene(path), oracle_mod.OracleScene(path)

    def rays(f):
        d_noise = to_dev(oracle_mod.noise_table(SEED, f))
        d_rays = to_dev(np.zeros(size[0] * size[1], oracle_mod.RAY_DTYPE))
        mrt_mod.raygen(sc, size[0], size[1], dev_ptr(d_noise), dev_ptr(d_rays), precise=True, camera=cam)
        return from_dev(d_rays, oracle_mod.RAY_DTYPE)
    ref = replay_render(oracle_mod, osc, size[0], size[1], L, FRAMES, rays)
    sc.close()
    rel, rmse, same = pixel_metrics(a, ref)
    print(f"stacked, moved camera vs replay: bit-identical {same:.5f}, rel<=1e-4 {np.mean(rel <= 1e-4):.5f}, "
          f"rmse {rmse:.2e}")
    assert ref[..., :3].max() > 0
    assert np.mean(rel <= 1e-4) >= 0.999 and rmse <= 1e-3
