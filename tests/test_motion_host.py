"""Host side of moving geometry (include/mrt.h mrt_scene_motion_compatible,
mrt_guides_motion): the compatibility check on host-only scenes, and the claim
the feature rests on, checked on the numpy model alone — mrt_reproject given the
MOTION planes (each pixel's surface point as it lay in the previous scene) in the
place of the current guide planes keeps the history of a block that moved, where
the current scene's own guide planes lose it."""
import numpy as np
import pytest

from denoise_model import NOT_FILTERABLE, guides_from_hits, words
from motion_cases import CENTRE, SHIFT, exchanged_obj, moved_obj, moved_prims, mtl_path
from temporal_cases import counted_image, fragile_limit
from temporal_model import reproject

ERR_INVALID = -1


def host_scene(mrt_mod, obj, mtl=None, **kw):
    return mrt_mod.Scene(obj, mtl, device=-1, **kw)


def test_compatible_pairs(mrt_mod, tmp_path):
    a = host_scene(mrt_mod, "cornellbox")
    moved = host_scene(mrt_mod, moved_obj(mrt_mod, tmp_path), mtl_path(mrt_mod))
    mrt_mod.scene_motion_compatible(a, moved)          # pair (a)
    mrt_mod.scene_motion_compatible(moved, a)
    mrt_mod.scene_motion_compatible(a, a)              # a scene with itself
    assert len(moved_prims(a.export(), moved.export())) == 12
    p1, p2 = (host_scene(mrt_mod, "cornellbox", procedural_triangles=512, procedural_seed=s) for s in (1, 2))
    mrt_mod.scene_motion_compatible(p1, p2)            # pair (b): the same topology, another surface
    assert len(moved_prims(p1.export(), p2.export())) > 256
    # builder options may differ
    mrt_mod.scene_motion_compatible(a, host_scene(mrt_mod, "cornellbox", max_leaf_size=2, occluder_tree=False))


def test_incompatible_pairs(mrt_mod, tmp_path):
    a = host_scene(mrt_mod, "cornellbox")
    with pytest.raises(mrt_mod.MrtError, match="triangles") as e:
        mrt_mod.scene_motion_compatible(a, host_scene(mrt_mod, "CornellBox-Water"))
    assert e.value.status == ERR_INVALID
    with pytest.raises(mrt_mod.MrtError, match="triangles") as e:
        mrt_mod.scene_motion_compatible(a, host_scene(mrt_mod, "cornellbox", procedural_triangles=512))
    assert e.value.status == ERR_INVALID
    # equal counts, two usemtl groups exchanged: the message names the first primitive that differs
    x = host_scene(mrt_mod, exchanged_obj(mrt_mod, tmp_path), mtl_path(mrt_mod))
    assert x.info["triangles"] == a.info["triangles"] and x.info["materials"] == a.info["materials"]
    ma, mx = a.export()["references"]["materialIndex"], x.export()["references"]["materialIndex"]
    k = int(np.flatnonzero(ma != mx)[0])
    with pytest.raises(mrt_mod.MrtError, match=f"primitive {k} has material") as e:
        mrt_mod.scene_motion_compatible(a, x)
    assert e.value.status == ERR_INVALID
    # the light group against a diffuse one of the same size: a light triangle in one scene only
    y = host_scene(mrt_mod, exchanged_obj(mrt_mod, tmp_path, "leftWall", "light", "cornellbox_light.obj"),
                   mtl_path(mrt_mod))
    la, ly = (s.export()["references"]["lightTriangleIndex"] != 0xFFFFFFFF for s in (a, y))
    assert np.array_equal(ma, y.export()["references"]["materialIndex"])     # (a material index is its group's rank)
    first = int(np.flatnonzero(la != ly)[0])
    with pytest.raises(mrt_mod.MrtError, match=f"primitive {first} is a light triangle in one scene only") as e:
        mrt_mod.scene_motion_compatible(a, y)
    assert e.value.status == ERR_INVALID
    assert mrt_mod.lib().mrt_scene_motion_compatible(None, a.handle) == ERR_INVALID


@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_motion_planes_keep_the_history_of_a_moved_block(mrt_mod, oracle_mod, tmp_path, W, H):
    """Pair (a) through the default camera, everything from the oracle.  A is the
    previous scene, B the current one (the block translated by SHIFT).  On the
    pixels that show the block in B:
      with the motion planes, history on at least 0.9 of them;
      with B's own guide planes in their place, on strictly fewer;
    and the fragile pixels of the motion case stay within fragile_limit.
    Measured: 64x48 block pixels 163, 1.000 with the motion planes against 0.092
    with B's guide planes, 40 fragile (limit 61); 37x29 block pixels 53, 1.000
    against 0.075, 14 fragile (limit 21).  (B's own positions project to where
    the block is NOW, where the old frame showed the floor, a wall or another
    face of the block, whose word or plane differ; the fragile pixels are those
    of an unmoved camera, whose fx and fy are integers but for rounding.)"""
    A = oracle_mod.OracleScene(mrt_mod.scene_path("cornellbox"))
    B = oracle_mod.OracleScene(moved_obj(mrt_mod, tmp_path), mtl_path(mrt_mod))
    rays = oracle_mod.raygen(W, H, CENTRE)
    hits_a, hits_b = A.intersect(rays), B.intersect(rays)
    ga = [g.reshape(H, W, 4) for g in guides_from_hits(A, hits_a, rays)]
    gb = [g.reshape(H, W, 4) for g in guides_from_hits(B, hits_b, rays)]
    motion = [g.reshape(H, W, 4) for g in guides_from_hits(A, hits_b, rays)]    # B's hits, A's vertices
    # the motion planes carry B's words and distances, and differ from B's planes exactly on the block
    assert np.array_equal(words(motion[0]), words(gb[0])) and np.array_equal(motion[1][..., 3], gb[1][..., 3])
    block = (np.isin(hits_b["triangleIndex"], moved_prims(A, B)) & (hits_b["distance"] >= 0)).reshape(H, W)
    assert block.sum() >= 50 and (words(gb[0])[block] < NOT_FILTERABLE).all()
    assert motion[1][~block].tobytes() == gb[1][~block].tobytes()
    moved = motion[1][block][:, :3].astype(np.float64) + np.array(SHIFT) - gb[1][block][:, :3]
    assert np.abs(moved).max() < 1e-5
    cam, params = mrt_mod.Camera.default(), mrt_mod.ReprojectParams.default()
    prev = counted_image(W, H, 100 * W + H)
    with_motion, fragile = reproject(prev, ga[0], ga[1], cam, motion[0], motion[1], params)
    static, _ = reproject(prev, ga[0], ga[1], cam, gb[0], gb[1], params)
    share_motion = float(np.mean(with_motion[..., 3][block] > 0))
    share_static = float(np.mean(static[..., 3][block] > 0))
    print(f"pair (a) {W}x{H}: block pixels {block.sum()}, history on {share_motion:.3f} of them with the motion planes, "
          f"{share_static:.3f} with the current guide planes; fragile {fragile.sum()} (limit {fragile_limit(W, H)})")
    assert share_motion >= 0.9
    assert share_motion > share_static
    assert fragile.sum() <= fragile_limit(W, H)
    # off the block the two agree wherever the old frame showed the same surface
    same = ~block & (hits_a["triangleIndex"] == hits_b["triangleIndex"]).reshape(H, W)
    assert with_motion[same].tobytes() == static[same].tobytes()
