"""CPU: the leaf-box sweep list (dev_sweep.h sweep_nearest) as
the host builds it — on the Cornell box and on generated rooms the list holds
every leaf of the main tree exactly once, each with the bits of the child box
its parent node holds, and the sweep is chosen exactly for trees of at most 32
leaves — and the wave-walk model (tools/walk_model.cpp) finds the two-phase
query's answers equal to the walk's on the Cornell box."""
import os
import subprocess

import numpy as np
import pytest

import roomgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32                      # mrt_layout.h kSweepLeaves
ROOMS = ["plain-1", "plain-4", "stacked", "float", "plain-5"]
EMPTY = 0x7FFFFFFF            # mrt_layout.h kEmptyChild


def _check_list(rec, info):
    """Structure of the list alone: one record per leaf, leaf refs distinct,
    their triangle ranges a partition of the leaf-ordered triangles, boxes
    lo <= hi, the padding word zero."""
    assert len(rec) == info["bvh_leaves"]
    refs = rec[:, 3].astype(np.uint32)
    assert (refs.view(np.int32) < 0).all() and len(set(refs.tolist())) == len(refs)
    lr = ~refs
    first, cnt = (lr >> 4).astype(np.int64), (lr & 15).astype(np.int64) + 1
    order = np.argsort(first)
    assert first[order][0] == 0 and (first[order][1:] == (first + cnt)[order][:-1]).all()
    assert (first + cnt).max() == info["triangles"]
    box = rec[:, [0, 1, 2, 4, 5, 6]].copy().view(np.float32)
    assert np.isfinite(box).all() and (box[:, :3] <= box[:, 3:]).all()
    assert (rec[:, 7] == 0).all()


def _cases(tmp_path):
    yield "cornellbox", "cornellbox"
    for name in ROOMS:
        yield name, roomgen.room(name, roomgen.seeds(name)[0], tmp_path).path


def test_sweep_list_holds_every_leaf_once_with_the_parents_box_bits(mrt_mod, tmp_path):
    seen_on, seen_off = 0, 0
    for name, obj in _cases(tmp_path):
        s = mrt_mod.Scene(obj, device=-1)
        enabled, rec = mrt_mod.debug_sweep_list(s)
        info = dict(s.info)
        nodes = mrt_mod.debug_bvh_nodes(s)
        s.close()
        print(f"{name}: {info['bvh_nodes']} nodes, {info['bvh_leaves']} leaves, {info['triangles']} triangles, "
              f"sweep {'on' if enabled else 'off'}, {len(rec)} records")
        # eligibility follows the cap; a tree over it keeps the walk and has no list
        assert enabled == (info["bvh_leaves"] <= CAP)
        if not enabled:
            assert len(rec) == 0
            seen_off += 1
            continue
        seen_on += 1
        _check_list(rec, info)
        # the records against the tree's own nodes: node order, slot order,
        # and the child's box rows bit for bit
        want = []
        for k in range(info["bvh_nodes"]):
            nd = nodes[k]
            for c in range(4):
                ref = int(nd[24 + c])
                if ref != EMPTY and ref >= 0x80000000:
                    want.append([nd[c], nd[8 + c], nd[16 + c], nd[24 + c], nd[4 + c], nd[12 + c], nd[20 + c], 0])
        assert np.array_equal(rec, np.array(want, np.uint32))
    assert seen_on >= 2 and seen_off >= 1   # plain-5 is over the cap


def test_sweep_switch_off_reports_the_walk(mrt_mod, monkeypatch):
    monkeypatch.setenv("MRT_SWEEP", "0")
    s = mrt_mod.Scene("cornellbox", device=-1)
    enabled, rec = mrt_mod.debug_sweep_list(s)
    s.close()
    assert not enabled and len(rec) == 22   # the list is built; the queries walk
    monkeypatch.delenv("MRT_DIAG")          # the switch is a diagnostic: ignored without MRT_DIAG=1
    s = mrt_mod.Scene("cornellbox", device=-1)
    enabled, _ = mrt_mod.debug_sweep_list(s)
    s.close()
    assert enabled


@pytest.fixture(scope="module")
def walk_model(tmp_path_factory):
    """tools/walk_model.cpp built by its own build line."""
    out = str(tmp_path_factory.mktemp("walk_model") / "walk_model")
    csrc = os.path.join(ROOT, "metal-renderer_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + csrc,
                    os.path.join(ROOT, "tools", "walk_model.cpp"), os.path.join(csrc, "scene.cpp"),
                    os.path.join(csrc, "bvh.cpp"), "-o", out, "-lpthread"], check=True)
    return out


def test_walk_model_finds_no_mismatch_on_the_cornell_box(mrt_mod, walk_model):
    r = subprocess.run([walk_model, mrt_mod.scene_path("cornellbox"), "200"], capture_output=True, text=True,
                       check=True)
    print(r.stdout)
    line = next(l for l in r.stdout.splitlines() if l.startswith("two-phase vs walk:"))
    rays, mismatches = int(line.split()[4]), int(line.split()[6])
    assert rays >= 200 * 64 and mismatches == 0
