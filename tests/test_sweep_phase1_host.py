"""CPU: phase 1's list of the leaf-box sweep (sweep_pairs.h
sweep_phase1_records) — one (centre, half-extent) record per
record of the list the kernels' phase 2 keeps, in its order and with its id
and mask bit; [c - e, c + e] contains the record's padded [lo, hi] on every
axis in exact (rational) arithmetic, with e the smallest float that does, two
ulps allowed; a scene that walks (MRT_SWEEP=0, or too many leaves) reports
none.  Scenes: the Cornell box (18 records) and generated rooms with 12
(plain-1), 18 (stacked) and 30 records (plain-4, next to the cap of 32).  Part 6
of the wave-walk model (tools/walk_model.cpp) finds the centre test
conservative on its camera blocks and adversarial rays."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import roomgen

SCENES = {"cornellbox": 18, "plain-1": 12, "stacked": 18, "plain-4": 30}
INELIGIBLE = "plain-5"


def _path(mrt_mod, name, tmp_path):
    if name == "cornellbox":
        return mrt_mod.scene_path(name)
    return roomgen.room(name, roomgen.seeds(name)[0], tmp_path).path


def _lists(mrt_mod, obj):
    """(enabled, pair records, phase-1 records) of a host-only scene, as uint32 views."""
    s = mrt_mod.Scene(obj, device=-1)
    enabled = mrt_mod.debug_sweep_list(s)[0]
    rec = mrt_mod.debug_sweep_pairs(s)[0]
    p1 = mrt_mod.debug_sweep_phase1(s)
    s.close()
    return enabled, rec, p1


def _ulps_above(x, y):
    """Floats from y up to x (both float32 >= 0): their bit patterns order as integers."""
    return int(np.float32(x).view(np.uint32)) - int(np.float32(y).view(np.uint32))


def _tightest(need):
    """The smallest float32 that is at least the rational `need` (>= 0)."""
    e = np.float32(float(need))
    while Fraction(float(e)) < need:
        e = np.nextafter(e, np.float32(np.inf))
    while e > 0 and Fraction(float(np.nextafter(e, np.float32(0)))) >= need:
        e = np.nextafter(e, np.float32(0))
    return e


@pytest.mark.parametrize("name", list(SCENES))
def test_one_entry_per_record_in_order_with_its_id(mrt_mod, tmp_path, name):
    enabled, rec, p1 = _lists(mrt_mod, _path(mrt_mod, name, tmp_path))
    print(f"{name}: {len(rec)} records, {len(p1)} phase-1 entries")
    assert enabled and len(rec) == SCENES[name] and len(p1) == len(rec)
    assert p1[:, 3].tolist() == list(range(len(rec)))
    assert p1[:, 7].tolist() == [1 << i for i in range(len(rec))]
    again = _lists(mrt_mod, _path(mrt_mod, name, tmp_path))
    assert p1.tobytes() == again[2].tobytes()


@pytest.mark.parametrize("name", list(SCENES))
def test_interval_contains_the_box_and_is_tight(mrt_mod, tmp_path, name):
    enabled, rec, p1 = _lists(mrt_mod, _path(mrt_mod, name, tmp_path))
    assert enabled and len(p1) == len(rec) == SCENES[name]
    lo, hi = rec[:, 0:3].view(np.float32), rec[:, 4:7].view(np.float32)
    c, e = p1[:, 0:3].view(np.float32), p1[:, 4:7].view(np.float32)
    assert np.isfinite(c).all() and np.isfinite(e).all() and (e >= 0).all()
    worst = 0
    for i in range(len(rec)):
        for a in range(3):
            L, H, C, E = (Fraction(float(v[i, a])) for v in (lo, hi, c, e))
            assert L <= H
            assert C - E <= L and C + E >= H, f"record {i} axis {a}: [{C - E}, {C + E}] misses [{L}, {H}]"
            over = _ulps_above(e[i, a], _tightest(max(C - L, H - C)))
            assert 0 <= over <= 2, f"record {i} axis {a}: e is {over} ulps above the tightest"
            worst = max(worst, over)
    print(f"{name}: e at most {worst} ulps above the tightest half-extent")


def test_walking_scenes_report_no_list(mrt_mod, tmp_path, monkeypatch):
    enabled, rec, p1 = _lists(mrt_mod, _path(mrt_mod, INELIGIBLE, tmp_path))
    assert not enabled and len(rec) == 0 and len(p1) == 0
    monkeypatch.setenv("MRT_SWEEP", "0")
    enabled, rec, p1 = _lists(mrt_mod, mrt_mod.scene_path("cornellbox"))
    assert not enabled and len(rec) == 18 and len(p1) == 0


@pytest.fixture(scope="module")
def walk_model(tmp_path_factory):
    """tools/walk_model.cpp built by its own build line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path_factory.mktemp("walk_model") / "walk_model")
    csrc = os.path.join(root, "metal-renderer_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + csrc,
                    os.path.join(root, "tools", "walk_model.cpp"), os.path.join(csrc, "scene.cpp"),
                    os.path.join(csrc, "bvh.cpp"), "-o", out, "-lpthread"], check=True)
    return out


def test_walk_model_part_6_finds_the_centre_test_conservative(mrt_mod, walk_model, tmp_path):
    """Part 6 of the wave-walk model: phase 1 on the centre list in the fast
    build's arithmetic gives the walk's (found, t, prim) on part 5's camera
    blocks and on the adversarial rays (with directions holding 0, -0 and
    +-1e-20 added); no record holding a triangle the ray hits is missed, and no
    key lies beyond such a triangle's cull bound.  Records the lo / hi test
    alone hits (an origin exactly on a padded face: that form's exact zeros)
    are printed, not capped: none of them holds a hit triangle."""
    for name, blocks in (("cornellbox", 200), ("stacked", 60), ("plain-4", 60)):
        r = subprocess.run([walk_model, _path(mrt_mod, name, tmp_path), str(blocks)], capture_output=True, text=True,
                           check=True)
        print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("6.", "   adversarial: 1", "phase 1 vs walk:"))))
        w = next(l for l in r.stdout.splitlines() if l.startswith("phase 1 vs walk:")).split()
        rays, bad, adv, adv_bad, with_hit, late = (int(w[k]) for k in (5, 7, 11, 13, 22, 26))
        assert rays >= blocks * 32 and adv >= 2000 and bad == 0 and adv_bad == 0 and with_hit == 0 and late == 0
