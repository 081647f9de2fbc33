"""GPU: the stream kernel's memory-wait changes (shadow roots as
named scalars, candidate-list headers and entries through scalar loads, a
wait the compiler sees before the survivor stores) change no pixel.  Fresh
scene and renderer per render, 3 frames, both builds:

a. the stream kernel is bitwise equal to the per-bounce kernels (MRT_STREAM=0),
   with equal active-ray counts;
b. the precise build is bit-identical to the oracle.

Shapes: the smallest at which a wrong list bound, a misplaced wait or a
changed queue order can show — path lengths with no queue level, one and
several, a ragged frame, a rank that owns the only tile and one that owns none
(every wave idle), a batch of one frame before a progressive draw, recycled
lanes returning to their level (MRT_SWEEP_CAP 0 and 3: the stores the new wait
precedes then include the recycle stores' own), a moved camera (the CAM = true
instantiation), and a camera whose candidate lists overflow their cap so that
every block falls back to the traversal.  Milliseconds per render, under a
second per oracle render."""
import numpy as np
import pytest

import roomgen
from helpers import SEED, pixel_metrics

pytestmark = pytest.mark.gpu

FRAMES = 3
ROOM = "stacked"


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return roomgen.room(ROOM, roomgen.seeds(ROOM)[0], tmp_path_factory.mktemp("gpu_stream_waits"))


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


def _render(mrt_mod, monkeypatch, path, size, L, precise, stream=True, shard=(0, 1), draws=(FRAMES,), cap=None,
            cam=None):
    """(image, stats) of a fresh scene and renderer."""
    monkeypatch.setenv("MRT_STREAM", "1" if stream else "0")
    if cap is None:
        monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    else:
        monkeypatch.setenv("MRT_SWEEP_CAP", str(cap))
    s = mrt_mod.Scene(path)
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise, shard_rank=shard[0], shard_count=shard[1])
    if cam is not None:
        r.set_camera(cam)
    for n in draws:
        r.draw(n)
    img, st = r.read_image(), r.stats()
    r.close()
    s.close()
    assert st["kernel"] == (2 if stream else 0)
    return img, st


def _check(mrt_mod, monkeypatch, path, size, L, what, ref=None, lit=True, **kw):
    """a. in both builds; b. against `ref` = (image, active rays) when given.
    Returns the stream renders' statistics (precise, fast)."""
    stats = []
    for precise in (True, False):
        a, sa = _render(mrt_mod, monkeypatch, path, size, L, precise, **kw)
        b, sb = _render(mrt_mod, monkeypatch, path, size, L, precise, stream=False, **{**kw, "cap": None})
        na, nb = sa["active_ray_bounces"], sb["active_ray_bounces"]
        same = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
        print(f"{what} {'precise' if precise else 'fast'}: stream vs per-bounce bit-identical {same:.5f}, "
              f"rays {na} / {nb}")
        assert np.isfinite(a).all() and (a[..., :3].max() > 0) == lit
        assert a.tobytes() == b.tobytes() and na == nb
        if precise and ref is not None:
            rel, rmse, same = pixel_metrics(a, ref[0])
            print(f"{what} precise vs oracle: bit-identical {same:.5f}, rmse {rmse:.2e}, rays {na} vs {ref[1]}")
            assert same == 1.0 and na == ref[1]
        stats.append(sa)
    return stats


@pytest.mark.parametrize("L", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
def test_cornell_box_stream_equals_per_bounce_and_oracle(gpu, mrt_mod, monkeypatch, reference, size, L):
    path = mrt_mod.scene_path("cornellbox")
    for st in _check(mrt_mod, monkeypatch, path, size, L, f"cornellbox {size[0]}x{size[1]} L={L}",
                     reference(path, size, L)):
        assert st["paths"] == size[0] * size[1] * FRAMES and st["primary_blocks"] > 0


@pytest.mark.parametrize("rank", [0, 3])
def test_tile_shard_with_and_without_a_tile(gpu, mrt_mod, monkeypatch, reference, rank):
    """64 x 48 is one 64 x 64 tile: of 8 ranks, rank 0 owns it (and renders
    the whole frame), rank 3 owns nothing — every wave of its launch is idle."""
    path, size, L = mrt_mod.scene_path("cornellbox"), (64, 48), 5
    ref = reference(path, size, L) if rank == 0 else None
    for st in _check(mrt_mod, monkeypatch, path, size, L, f"rank {rank} of 8", ref, lit=rank == 0, shard=(rank, 8)):
        assert st["paths"] == (size[0] * size[1] * FRAMES if rank == 0 else 0)
        assert (st["active_ray_bounces"] > 0) == (rank == 0)


def test_batch_of_one_then_progressive(gpu, mrt_mod, monkeypatch, reference):
    """A draw of one frame (a batch of 1), then a draw of two: the wave queues
    are reused by the second draw's launch."""
    path, size, L = mrt_mod.scene_path("cornellbox"), (97, 61), 5
    for st in _check(mrt_mod, monkeypatch, path, size, L, "draws 1 + 2", reference(path, size, L), draws=(1, 2)):
        assert st["paths"] == size[0] * size[1] * FRAMES and st["kernel_launches"] == 2


@pytest.mark.parametrize("cap", [0, 3])
def test_recycled_lanes_return_to_their_level(gpu, mrt_mod, monkeypatch, reference, cap):
    """Under a cap a pass recycles lanes onto the level it ran; the per-bounce
    kernels never recycle."""
    path, size, L = mrt_mod.scene_path("cornellbox"), (97, 61), 5
    monkeypatch.setenv("MRT_SWEEP_CAP", str(cap))
    s = mrt_mod.Scene(path)
    on, got = mrt_mod.debug_sweep_list(s)[0], mrt_mod.debug_sweep_cap(s)
    s.close()
    assert on and got == cap
    _check(mrt_mod, monkeypatch, path, size, L, f"cap {cap}", reference(path, size, L), cap=cap)


def _low_camera(mrt_mod, rm):
    """0.06 off a top corner of the room's first block, looking along its top
    towards the opposite corner (test_gpu_rooms' edge camera): its plane cuts
    more triangles than the candidate lists' cap."""
    P = rm.blocks[0]
    out = P[4] - P[4:].mean(0)
    eye = P[4] + 0.06 * out / np.linalg.norm(out) + np.array([0.0, 0.03, 0.0])
    target = P[6] - np.array([0.0, 0.1, 0.0])
    return mrt_mod.Camera.look_at(tuple(eye), tuple(target), (0.0, 1.0, 0.0), 70.0)


def test_moved_camera_in_a_room(gpu, mrt_mod, monkeypatch, room):
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    for st in _check(mrt_mod, monkeypatch, room.path, (97, 61), 4, f"{ROOM}, moved camera", cam=cam):
        assert st["primary_blocks"] > 0


def test_candidate_lists_over_their_cap_fall_back(gpu, mrt_mod, monkeypatch, room):
    for st in _check(mrt_mod, monkeypatch, room.path, (97, 61), 4, f"{ROOM}, low camera",
                     cam=_low_camera(mrt_mod, room)):
        assert st["primary_blocks"] == 0
