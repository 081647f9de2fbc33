"""GPU: phase 1 of the nearest sweep with its bookkeeping in the lanes that
hit only and, in the fast build, the centre / half-extent slab test on a list
of its own (dev_sweep.h sweep_nearest / sweep_centre) changes no
pixel.  Fresh scene and renderer per render, 3 frames, both builds:

a. the sweep is bitwise equal, image and active-ray count, to MRT_SWEEP=0 (the
   walk, which shares none of phase 1);
b. the stream kernel is bitwise equal to the per-bounce kernels (MRT_STREAM=0),
   which inline the same sweep;
c. the precise build is bit-identical to the oracle.

Shapes: the Cornell box (18 records) and rooms with 12, 18 and 30 records (the
last next to the cap of 32: the mask's high bits), 64 x 48 and a ragged
97 x 61, L = 2, 3 and 5 (one and several swept levels, with the last-bounce
shortcut behind them); once a moved camera
(the CAM = true instantiation, origins inside record boxes) and once
MRT_SWEEP_CAP=0 (resumed lanes ride through phase 1 and ignore its keys).
Milliseconds per render, under a second per oracle render."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 3
SCENES = {"cornellbox": 18, "plain-1": 12, "stacked": 18, "plain-4": 30}


@pytest.fixture(scope="module")
def scene(mrt_mod, tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_sweep_phase1"), {}

    def get(name):
        if name not in cache:
            cache[name] = (mrt_mod.scene_path(name) if name == "cornellbox"
                           else roomgen.room(name, roomgen.seeds(name)[0], d).path)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(image, active rays) of the oracle, rendered once per (scene, size, L)."""
    cache = {}

    def get(path, size, L):
        key = (path, size, L)
        if key not in cache:
            cache[key] = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
            assert np.isfinite(cache[key][0]).all() and cache[key][0][..., :3].max() > 0
        return cache[key]
    return get


def _render(mrt_mod, monkeypatch, path, size, L, precise, sweep=True, stream=True, cap=None, cam=None):
    """(image, active ray bounces, sweep enabled, phase-1 entries) of a fresh scene and renderer."""
    monkeypatch.setenv("MRT_SWEEP", "1" if sweep else "0")
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    if cap is None:
        monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    else:
        monkeypatch.setenv("MRT_SWEEP_CAP", str(cap))
    s = mrt_mod.Scene(path)
    enabled, entries = mrt_mod.debug_sweep_list(s)[0], len(mrt_mod.debug_sweep_phase1(s))
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise)
    if cam is not None:
        r.set_camera(cam)
    r.draw(FRAMES)
    img, st = r.read_image(), r.stats()
    r.close()
    s.close()
    assert st["kernel"] == (2 if stream else 0) and st["paths"] == size[0] * size[1] * FRAMES
    return img, st["active_ray_bounces"], enabled, entries


def _check(mrt_mod, monkeypatch, path, size, L, records, what, ref=None, cap=None, cam=None):
    for precise in (True, False):
        build = "precise" if precise else "fast"
        a, na, on, entries = _render(mrt_mod, monkeypatch, path, size, L, precise, cap=cap, cam=cam)
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


@pytest.mark.parametrize("L", [2, 3, 5])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
@pytest.mark.parametrize("name", list(SCENES))
def test_sweep_equals_walk_per_bounce_and_oracle(gpu, mrt_mod, monkeypatch, scene, reference, name, size, L):
    path = scene(name)
    _check(mrt_mod, monkeypatch, path, size, L, SCENES[name], f"{name} {size[0]}x{size[1]} L={L}",
           ref=reference(path, size, L))


def test_moved_camera_inside_the_room(gpu, mrt_mod, monkeypatch, scene):
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    _check(mrt_mod, monkeypatch, scene("plain-4"), (97, 61), 5, SCENES["plain-4"], "plain-4, moved camera", cam=cam)


def test_resumed_lanes_ignore_their_keys(gpu, mrt_mod, monkeypatch, scene, reference):
    """MRT_SWEEP_CAP=0: every lane with a record left after the key rounds is
    recycled, rides through phase 1 again and pops its mask in the key rounds."""
    path, size, L = scene("cornellbox"), (97, 61), 5
    monkeypatch.setenv("MRT_SWEEP_CAP", "0")
    s = mrt_mod.Scene(path)
    got = mrt_mod.debug_sweep_cap(s)
    s.close()
    assert got == 0
    _check(mrt_mod, monkeypatch, path, size, L, SCENES["cornellbox"], "cornellbox, cap 0",
           ref=reference(path, size, L), cap=0)
