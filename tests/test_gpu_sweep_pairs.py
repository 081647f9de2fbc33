"""GPU: the sweep over triangle-pair records with the culled-key early-out and
the third key (dev_sweep.h sweep_nearest) returns the walk's
answer — on the Cornell box (64 x 48 and a ragged 97 x 61, L = 3, 4, 5: a
shorter path has no swept bounce) and on generated rooms (96 x 64, L = 4),
3 frames, in both builds:

a. the default is bitwise equal, image and active-ray count, to MRT_SWEEP=0
   (the walk) and to MRT_SWEEP_PAIRS=0 (one record per leaf);
b. the stream kernel is bitwise equal to the per-bounce kernels;
c. MRT_SWEEP_CAP 0 and 3 (recycled rays: resumed lanes pop in the key rounds
   and never take the early-out) are bitwise equal to the uncapped default;
d. the precise build is bit-identical to the oracle.

One eligible room is rendered through a moved camera (a. to c.).
Milliseconds per render, under a second per oracle render."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 3
ROOMS = ["plain-1", "plain-3", "stacked", "float"]


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_sweep_pairs"), {}

    def get(name):
        if name not in cache:
            cache[name] = roomgen.room(name, roomgen.seeds(name)[0], d).path
        return cache[name]
    return get


def _render(mrt_mod, monkeypatch, path, size, L, precise, sweep=True, pairs=True, stream=True, cap=None, cam=None):
    """(image, active ray bounces, sweep enabled, records) of a fresh scene and renderer."""
    monkeypatch.setenv("MRT_SWEEP", "1" if sweep else "0")
    monkeypatch.setenv("MRT_SWEEP_PAIRS", "1" if pairs else "0")
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    if cap is None:
        monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    else:
        monkeypatch.setenv("MRT_SWEEP_CAP", str(cap))
    s = mrt_mod.Scene(path)
    enabled, leaves = mrt_mod.debug_sweep_list(s)
    rec, _ = mrt_mod.debug_sweep_pairs(s)
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise)
    if cam is not None:
        r.set_camera(cam)
    r.draw(FRAMES)
    img, st = r.read_image(), r.stats()
    r.close()
    s.close()
    assert st["kernel"] == (2 if stream else 0) and st["paths"] == size[0] * size[1] * FRAMES
    assert len(rec) <= len(leaves) if pairs else len(rec) == len(leaves)
    return img, st["active_ray_bounces"], enabled, len(rec)


def _check(mrt_mod, monkeypatch, path, size, L, ref=None, cam=None, what=""):
    for precise in (True, False):
        build = "precise" if precise else "fast"
        a, na, on, recs = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam)
        assert on and np.isfinite(a).all() and a[..., :3].max() > 0
        for other, kw in (("walk", dict(sweep=False)), ("one record per leaf", dict(pairs=False)),
                          ("per-bounce kernels", dict(stream=False)), ("cap 0", dict(cap=0)), ("cap 3", dict(cap=3))):
            b, nb, on_b, recs_b = _render(mrt_mod, monkeypatch, path, size, L, precise, cam=cam, **kw)
            assert on_b == (other != "walk")
            same = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
            print(f"{what} {build}: {recs} records, default vs {other} ({recs_b} records): bit-identical {same:.5f}, "
                  f"rays {na} / {nb}")
            assert a.tobytes() == b.tobytes() and na == nb
        if precise and ref is not None:
            rel, rmse, same = pixel_metrics(a, ref[0])
            print(f"{what} precise vs oracle: bit-identical {same:.5f}, rmse {rmse:.2e}, rays {na} vs {ref[1]}")
            assert same == 1.0 and na == ref[1]


@pytest.mark.parametrize("L", [3, 4, 5])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
def test_cornell_box_pairs_equal_walk_and_oracle(gpu, mrt_mod, oracle_mod, monkeypatch, size, L):
    path = mrt_mod.scene_path("cornellbox")
    ref = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
    assert np.isfinite(ref[0]).all() and ref[0][..., :3].max() > 0
    _check(mrt_mod, monkeypatch, path, size, L, ref, what=f"cornellbox {size[0]}x{size[1]} L={L}")


@pytest.mark.parametrize("name", ROOMS)
def test_rooms_pairs_equal_walk_and_oracle(gpu, mrt_mod, oracle_mod, monkeypatch, room, name):
    path, size, L = room(name), (96, 64), 4
    ref = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
    assert np.isfinite(ref[0]).all() and ref[0][..., :3].max() > 0
    _check(mrt_mod, monkeypatch, path, size, L, ref, what=name)


def test_moved_camera_pairs_equal_walk(gpu, mrt_mod, monkeypatch, room):
    """An eligible room through a camera inside it (the kernels' CAM = true
    instantiation; origins inside record boxes)."""
    path, size, L = room("stacked"), (97, 61), 4
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    _check(mrt_mod, monkeypatch, path, size, L, cam=cam, what="stacked, moved camera")
