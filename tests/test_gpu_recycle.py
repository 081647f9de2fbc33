"""GPU: the stream kernel's capped sweep with recycled rays (kern_bounce.h
bounce_wave / sweep_nearest) changes no result.  A ray's answer
is the minimum of (t, prim) over the same tested leaves under the same cull
rule whatever pass tests them, so on the Cornell box (64 x 48 and a ragged
70 x 50) and on the generated room with a full 32-leaf mask, at L = 1, 2, 4, 5,
in both builds, for a 3-frame batch and for two successive draws:

a. the default (the product never recycles: every cap measured slower) is
   bitwise equal — image and active-ray count — to MRT_SWEEP_CAP=3 (the
   model's pick), to MRT_SWEEP=0 (the walk), and to MRT_SWEEP_CAP=0, where
   every ray that needs a rest pop goes back on its queue, some of them
   several times, and a level refills to its bound;
b. the precise build is bit-identical to the oracle at 64 x 48, L = 4, under
   the default and under both caps.

Milliseconds per render, under a second for the oracle's."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 3
UNCAPPED = 32                 # mrt_layout.h kSweepLeaves
ROOM = "plain-4"              # 32 leaves: every bit of a lane's mask, leaf 31 included
CASES = [("cornellbox", (64, 48)), ("cornellbox", (70, 50)), (ROOM, (64, 48))]


@pytest.fixture(scope="module")
def scene_path(mrt_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_recycle")
    room = roomgen.room(ROOM, roomgen.seeds(ROOM)[0], d).path
    return lambda name: room if name == ROOM else mrt_mod.scene_path(name)


def _render(mrt_mod, monkeypatch, path, size, L, precise, cap=None, sweep=True):
    """((batch image, rays), (image, rays) after two draws, sweep on, cap) of a fresh scene."""
    monkeypatch.setenv("MRT_SWEEP", "1" if sweep else "0")
    if cap is None:
        monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    else:
        monkeypatch.setenv("MRT_SWEEP_CAP", str(cap))
    s = mrt_mod.Scene(path)
    on, _ = mrt_mod.debug_sweep_list(s)
    got_cap = mrt_mod.debug_sweep_cap(s)
    out = []
    for draws in ((FRAMES,), (2, 1)):
        r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise)
        for n in draws:
            r.draw(n)
        img, st = r.read_image(), r.stats()
        r.close()
        assert st["kernel"] == 2 and st["paths"] == size[0] * size[1] * FRAMES
        out.append((img, st["active_ray_bounces"]))
    s.close()
    return out[0], out[1], on, got_cap


@pytest.mark.parametrize("L", [1, 2, 4, 5])
@pytest.mark.parametrize("name,size", CASES)
def test_recycling_changes_no_pixel_and_no_ray_count(gpu, mrt_mod, oracle_mod, monkeypatch, scene_path, name, size, L):
    path = scene_path(name)
    for precise in (True, False):
        build = "precise" if precise else "fast"
        b0, d0, on, cap = _render(mrt_mod, monkeypatch, path, size, L, precise)
        assert on and cap == UNCAPPED, "the product sweeps this scene and never recycles"
        assert np.isfinite(b0[0]).all() and b0[0][..., :3].max() > 0
        against_oracle = [("default", b0)]
        for what, kw in (("cap 3", dict(cap=3)), ("walk", dict(sweep=False)), ("cap 0", dict(cap=0))):
            b, d, on_v, cap_v = _render(mrt_mod, monkeypatch, path, size, L, precise, **kw)
            assert on_v == (what != "walk") and cap_v == kw.get("cap", UNCAPPED)
            for how, (x, nx), (y, ny) in (("batch", b0, b), ("two draws", d0, d)):
                same = (x.view(np.uint32) == y.view(np.uint32)).all(-1).mean()
                print(f"{name} {size[0]}x{size[1]} L={L} {build}, default vs {what}, {how}: "
                      f"bit-identical {same:.5f}, rays {nx} / {ny}")
                assert x.tobytes() == y.tobytes() and nx == ny
            against_oracle.append((what, b))
        if precise and name == "cornellbox" and size == (64, 48) and L == 4:
            ref, rays = oracle_mod.OracleScene(path).render(size[0], size[1], L, SEED, FRAMES, threads=8)
            assert ref[..., :3].max() > 0
            for what, (img, n) in against_oracle:
                rel, rmse, same = pixel_metrics(img, ref)
                print(f"precise, {what} vs oracle: bit-identical {same:.5f}, rmse {rmse:.2e}, rays {n} vs {rays}")
                assert same == 1.0 and n == rays
