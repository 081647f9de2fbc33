"""CPU: the detectors (csrc/occluders.cpp find_occluders and
find_convex_occluders) on every generated room of tests/roomgen.py: the
number of convex solids found, whether the occluder tree is built, and the
host tree check — plus the generator's own promises (deterministic, the room's
extent, float32-exact coordinates)."""
import numpy as np
import pytest

import roomgen


@pytest.mark.parametrize("name,seed", [(n, s) for n in sorted(roomgen.CASES) for s in roomgen.seeds(n)])
def test_detection_on_generated_rooms(mrt_mod, tmp_path, name, seed):
    rm = roomgen.room(name, seed, tmp_path)
    s = mrt_mod.Scene(rm.path, device=-1)
    info = dict(s.info)
    print(rm.id, {k: info[k] for k in ("convex_solids", "occluder_planes", "occluder_culled", "occluder_margin",
                                       "occluder_cos_min")})
    assert info["convex_solids"] == rm.convex_solids
    assert (info["occluder_planes"] > 0) == rm.occluder_tree
    assert info["occluder_planes"] == 5   # floor, ceiling, back, left and right walls
    s.check_bvh()
    e = s.export()
    lights = int((e["references"]["lightTriangleIndex"] != 0xFFFFFFFF).sum())
    assert lights == (4 if name == "twolights" else 2)
    V = e["vertices"]["v"]
    assert (V.min(0) == (-1, 0, -1)).all() and (V.max(0) == (1, 2, 1)).all()
    s.close()
    off = mrt_mod.Scene(rm.path, device=-1, occluder_tree=False)
    assert off.info["occluder_planes"] == 0 and off.info["convex_solids"] == 0
    off.close()


def test_deeper_occluder_tree_is_dropped(mrt_mod, tmp_path):
    """float, seed 1: the occluder tree needs a deeper stack (8) than the main
    tree (7), so the library keeps only the main tree — no planes, no solids —
    and the tree check still passes."""
    s = mrt_mod.Scene(roomgen.room("float", 1, tmp_path).path, device=-1)
    assert s.info["occluder_planes"] == 0 and s.info["occluder_nodes"] == 0 and s.info["convex_solids"] == 0
    s.check_bvh()
    s.close()


def test_rooms_are_reproducible(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    for name in roomgen.CASES:
        ra, rb = roomgen.room(name, 3, a), roomgen.room(name, 3, b)
        assert open(ra.path).read() == open(rb.path).read()
        assert open(ra.path).read() != open(roomgen.room(name, 4, b).path).read()
        # every coordinate is a float32 value written with 9 significant digits (it round-trips)
        for line in open(ra.path):
            w = line.split()
            if w and w[0] in ("v", "vn"):
                for t in w[1:]:
                    assert "%.9g" % float(np.float32(float(t))) == t, line
