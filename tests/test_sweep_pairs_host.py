"""CPU: the list the sweep kernels get (sweep_pairs.h) — one
record per group of at most two triangles, derived from the per-leaf list:
every triangle of the tree in exactly one record, each record's box the
min / max of its members' boxes as their parent nodes hold them, never more
records than leaves, the same bytes from two creations, the Cornell box's
four pairs, the no-pair room unchanged, the ceil(cnt / 2) rule for larger
leaves, the MRT_SWEEP_PAIRS=0 switch — and part 5 of the wave-walk model
(tools/walk_model.cpp) finds the paired list, the culled-key early-out and
the third key equal to the walk, its adversarial rays included."""
import os
import subprocess

import numpy as np
import pytest

import roomgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOMS = ["plain-1", "plain-3", "plain-4", "stacked", "float", "plain-5"]
INELIGIBLE = "plain-5"
EMPTY = 0x7FFFFFFF            # mrt_layout.h kEmptyChild


def _room(name, tmp_path):
    return roomgen.room(name, roomgen.seeds(name)[0], tmp_path).path


def _lists(mrt_mod, obj, **kw):
    """(info, nodes, per-leaf records, pair records, pair prims) of a host-only scene."""
    s = mrt_mod.Scene(obj, device=-1, **kw)
    enabled, leaves = mrt_mod.debug_sweep_list(s)
    rec, prims = mrt_mod.debug_sweep_pairs(s)
    info, nodes = dict(s.info), mrt_mod.debug_bvh_nodes(s)
    s.close()
    return info, nodes, enabled, leaves, rec, prims


def _leaf_boxes(nodes):
    """[(first, cnt, lo[3], hi[3])] of the tree's leaves, from its nodes."""
    out = []
    for nd in nodes:
        f = nd.view(np.float32)
        for c in range(4):
            ref = int(nd[24 + c])
            if ref != EMPTY and ref >= 0x80000000:
                lr = ~ref & 0xFFFFFFFF
                out.append((lr >> 4, (lr & 15) + 1, f[[c, 8 + c, 16 + c]], f[[4 + c, 12 + c, 20 + c]]))
    return out


def _check_records(info, nodes, leaves, rec):
    """Every triangle once; each box the min / max of its members' leaf boxes;
    a leaf of more than two triangles in ceil(cnt / 2) records of its own."""
    ka, kb = (rec[:, 3] & 0xFFFF).astype(np.int64), (rec[:, 3] >> 16).astype(np.int64)
    tris = sorted(ka.tolist() + kb[kb != ka].tolist())
    assert tris == list(range(info["triangles"]))
    assert (rec[:, 7] == 0).all() and len(rec) <= len(leaves)
    boxes = _leaf_boxes(nodes)

    def leaf_of(k):
        return next(b for b in boxes if b[0] <= k < b[0] + b[1])
    recs_of_leaf = {}
    for i in range(len(rec)):
        a, b = leaf_of(ka[i]), leaf_of(kb[i])
        lo, hi = np.minimum(a[2], b[2]), np.maximum(a[3], b[3])
        got = rec[i].view(np.float32)
        assert np.array_equal(got[[0, 1, 2]], lo) and np.array_equal(got[[4, 5, 6]], hi)
        if a[0] != b[0]:
            assert a[1] == 1 and b[1] == 1    # only single-triangle leaves share a record
        else:
            recs_of_leaf[a[0]] = recs_of_leaf.get(a[0], 0) + 1
    for first, cnt, _, _ in boxes:
        if first in recs_of_leaf:
            assert recs_of_leaf[first] == (cnt + 1) // 2


def test_pair_list_partitions_the_triangles_with_union_boxes(mrt_mod, tmp_path):
    seen = 0
    for name in ["cornellbox"] + ROOMS:
        obj = "cornellbox" if name == "cornellbox" else _room(name, tmp_path)
        info, nodes, enabled, leaves, rec, prims = _lists(mrt_mod, obj)
        again = _lists(mrt_mod, obj)
        print(f"{name}: {info['bvh_leaves']} leaves, {len(rec)} records, sweep {'on' if enabled else 'off'}")
        assert rec.tobytes() == again[4].tobytes() and prims.tobytes() == again[5].tobytes()
        if name == INELIGIBLE:
            assert not enabled and len(rec) == 0 and len(leaves) == 0
            continue
        assert enabled and len(leaves) == info["bvh_leaves"]
        _check_records(info, nodes, leaves, rec)
        seen += 1
    assert seen == len(ROOMS)


def test_cornell_box_pairs_its_blocks_tops_and_bottoms(mrt_mod):
    info, nodes, enabled, leaves, rec, prims = _lists(mrt_mod, "cornellbox")
    assert enabled and len(leaves) == 22 and len(rec) == 18
    boxes = {b[0]: b[1] for b in _leaf_boxes(nodes)}
    ka, kb = rec[:, 3] & 0xFFFF, rec[:, 3] >> 16
    joined = {frozenset(p.tolist()) for p, a, b in zip(prims, ka, kb) if boxes.get(int(a)) == 1 and a != b}
    assert joined == {frozenset(s) for s in ((34, 35), (24, 25), (22, 23), (12, 13))}


def test_room_without_single_leaves_keeps_its_list(mrt_mod, tmp_path):
    info, nodes, enabled, leaves, rec, prims = _lists(mrt_mod, _room("plain-1", tmp_path))
    assert enabled and len(leaves) == 12 and len(rec) == 12
    # the no-pair path: record i is leaf i with its box
    assert np.array_equal(rec[:, [0, 1, 2, 4, 5, 6, 7]], leaves[:, [0, 1, 2, 4, 5, 6, 7]])


def test_larger_leaves_split_into_pairs(mrt_mod):
    info, nodes, enabled, leaves, rec, prims = _lists(mrt_mod, "cornellbox", max_leaf_size=4)
    cnts = [b[1] for b in _leaf_boxes(nodes)]
    print(f"max_leaf_size 4: leaf sizes {sorted(cnts)}, {len(rec)} records")
    assert max(cnts) > 2 and len(leaves) == len(cnts)
    _check_records(info, nodes, leaves, rec)
    singles = sum(1 for c in cnts if c == 1)
    assert sum((c + 1) // 2 for c in cnts) - singles // 2 <= len(rec) <= sum((c + 1) // 2 for c in cnts)


def test_pairs_switch_gives_one_record_per_leaf(mrt_mod, monkeypatch):
    monkeypatch.setenv("MRT_SWEEP_PAIRS", "0")
    info, nodes, enabled, leaves, rec, prims = _lists(mrt_mod, "cornellbox")
    assert enabled and len(rec) == 22
    _check_records(info, nodes, leaves, rec)
    assert np.array_equal(rec[:, [0, 1, 2, 4, 5, 6]], leaves[:, [0, 1, 2, 4, 5, 6]])
    monkeypatch.delenv("MRT_DIAG")          # the switch is a diagnostic: ignored without MRT_DIAG=1
    assert len(_lists(mrt_mod, "cornellbox")[4]) == 18


@pytest.fixture(scope="module")
def walk_model(tmp_path_factory):
    """tools/walk_model.cpp built by its own build line."""
    out = str(tmp_path_factory.mktemp("walk_model") / "walk_model")
    csrc = os.path.join(ROOT, "metal-renderer_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + csrc,
                    os.path.join(ROOT, "tools", "walk_model.cpp"), os.path.join(csrc, "scene.cpp"),
                    os.path.join(csrc, "bvh.cpp"), "-o", out, "-lpthread"], check=True)
    return out


def _part5(stdout):
    line = next(l for l in stdout.splitlines() if l.startswith("pairs vs walk:"))
    w = line.split()
    return int(w[4]), int(w[6]), int(w[10]), int(w[12])   # rays, mismatches, adversarial rays, mismatches


def test_walk_model_part_5_finds_no_mismatch(mrt_mod, walk_model, tmp_path):
    for obj, blocks in ((mrt_mod.scene_path("cornellbox"), 200), (_room("plain-3", tmp_path), 60),
                        (_room("stacked", tmp_path), 60)):
        r = subprocess.run([walk_model, obj, str(blocks)], capture_output=True, text=True, check=True)
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("5.", "   ", "pairs vs walk:"))))
        rays, bad, adv, adv_bad = _part5(r.stdout)
        assert rays >= blocks * 32 and adv >= 1000 and bad == 0 and adv_bad == 0
