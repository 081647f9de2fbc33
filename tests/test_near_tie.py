"""The traversal's culling slack against the near tie of DESIGN.md §3.1.

The kernels cull a BVH4 child only when its slab entry lies beyond the current
hit's t by more than 2^-11 of it (dev_traverse.h kCullScale).  The committed
regression ray (tests/golden/near_tie_ray.json) is the one that made a C5
pixel differ between identical renders before that slack: the fast build's
triangle test put prim 7787 at a t 1.85e-5 (relative) before 7787's own
padded leaf box.  The CPU tests pin, over the product's own BVH4 (host-built,
no device; libmrt's test entry mrt_debug_box_margin):
  * the oracle's brute force, its wide-slack CPU BVH and its no-cull CPU BVH
    agree on the ray (IEEE: prim 9834);
  * the box excess of the fast build's hit is positive (the failure mode) and
    below the kernels' slack (the fix covers it), and the rounding envelope of
    the IEEE hit's near ties covers that hit;
  * on real rays of the 1M-triangle scene (every bounce of a 64x48 frame), the
    oracle's BVH with and without culling equals its brute force bitwise.
The GPU test asks mrt_intersect (the B-2 stage, both builds) for the ray in
every lane position of a wave among other rays: the precise build returns the
oracle's answer bit for bit, the fast build one answer whatever the position."""
import json
import os
import struct

import numpy as np
import pytest

from helpers import GOLDEN, SEED, dev_ptr, from_dev, to_dev

VEC = json.load(open(os.path.join(GOLDEN, "near_tie_ray.json")))


def _f(h):
    return struct.unpack("<f", struct.pack("<I", int(h, 16)))[0]


@pytest.fixture(scope="module")
def tie_scene(mrt_mod, oracle_mod):
    s = VEC["scene"]
    sc = mrt_mod.Scene(s["obj"], procedural_triangles=s["procedural_triangles"], procedural_seed=s["procedural_seed"],
                       device=-1)
    e = sc.export()
    osc = oracle_mod.OracleScene.from_arrays(e["vertices"], e["references"], e["materials"])
    yield sc, osc
    sc.close()


def _ray(oracle_mod, n=1):
    r = np.zeros(n, oracle_mod.RAY_DTYPE)
    r["origin"][:] = [_f(h) for h in VEC["origin_bits"]]
    r["direction"][:] = [_f(h) for h in VEC["direction_bits"]]
    r["maxDistance"] = np.inf
    return r


def _tbits(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def test_near_tie_ray_oracle_traversals_agree(tie_scene, oracle_mod):
    sc, osc = tie_scene
    r = _ray(oracle_mod)
    want = VEC["ieee_hit"]
    for name, got in (("brute force", osc.intersect(r)), ("CPU BVH", osc.intersect_bvh(r)),
                      ("CPU BVH, no culling", osc.intersect_bvh(r, nocull=True))):
        assert int(got["triangleIndex"][0]) == want["prim"], name
        assert _tbits(got["distance"][0]) == want["t_bits"], name


def test_near_tie_ray_box_excess_within_slack(tie_scene, oracle_mod):
    sc, osc = tie_scene
    r = _ray(oracle_mod)
    slack = VEC["kernel_cull_slack"]
    assert slack == 2.0 ** -11
    # the fast build's answer 7787 at its own t: entered only after the hit —
    # the failure mode — but within the slack, so no order can lose it now
    hit = osc.intersect(r)
    fast = hit.copy()
    fast["triangleIndex"] = VEC["fast_build_hits"][0]["prim"]
    fast["distance"] = _f(VEC["fast_build_hits"][0]["t_bits"])
    m = sc.box_margin(r, fast)[0]
    assert m[0] == pytest.approx(VEC["box_entry_excess_7787_at_fast_t"], rel=1e-3) and m[1] == m[0]
    assert 0 < m[0] < slack / 16
    # the IEEE hit (9834): its own boxes are entered before it; its near ties
    # (7787 within the rounding envelope) need at least the fast build's
    # excess and still less than the slack
    m = sc.box_margin(r, hit)[0]
    assert m[0] < 0 and m[1] < 0
    assert VEC["box_entry_excess_7787_at_fast_t"] <= m[2] < slack and m[3] < slack


def test_cpu_bvh_culling_modes_equal_bruteforce_on_1m_scene(tie_scene, oracle_mod):
    """Every path and shadow ray of a 64x48 frame (L = 4) of the 1M-triangle
    scene: brute force == the CPU BVH with its wide slack == without culling,
    bit for bit (the wide-slack tree is what the full-size parity tests and
    the bench's parity leg compare the kernels with)."""
    sc, osc = tie_scene
    W, H, L, f = 64, 48, 4, 3
    rays = oracle_mod.raygen(W, H, oracle_mod.noise_table(SEED, f))
    n_cmp = 0
    for i in range(L):
        noise = oracle_mod.noise_table(SEED, oracle_mod.noise_frame_for(f, i))
        ref = osc.intersect(rays)
        for nocull in (False, True):
            got = osc.intersect_bvh(rays, threads=4, nocull=nocull)
            assert got.tobytes() == ref.tobytes(), (i, nocull)
        srays = np.zeros(len(rays), oracle_mod.SRAY_DTYPE)
        osc.shade(W, H, f, L, noise, ref, rays, srays)
        sref = osc.intersect(srays)
        for nocull in (False, True):
            assert osc.intersect_bvh(srays, threads=4, nocull=nocull).tobytes() == sref.tobytes(), (i, nocull)
        oracle_mod.resolve(sref, rays, srays)
        n_cmp += 2 * len(rays)
    assert n_cmp == 2 * L * W * H


@pytest.mark.gpu
def test_near_tie_ray_through_mrt_intersect(gpu, mrt_mod, oracle_mod):
    s = VEC["scene"]
    sc = mrt_mod.Scene(s["obj"], procedural_triangles=s["procedural_triangles"], procedural_seed=s["procedural_seed"])
    e = sc.export()
    osc = oracle_mod.OracleScene.from_arrays(e["vertices"], e["references"], e["materials"])
    # the ray at every lane position of a 64-lane wave, the other lanes holding
    # camera rays (which finish early) or copies of the ray itself
    cams = oracle_mod.raygen(64, 64, oracle_mod.noise_table(SEED, 0))
    rays = cams.copy()
    tie = _ray(oracle_mod)[0]
    pos = np.arange(0, len(rays), 67)   # every lane slot, many waves
    rays[pos] = tie
    rays[-64:] = tie                    # one wave of nothing but the ray
    pos = np.concatenate([pos, np.arange(len(rays) - 64, len(rays))])
    ref = osc.intersect(rays)
    for precise in (True, False):
        d_rays = to_dev(rays)
        d_out = to_dev(np.zeros(len(rays), oracle_mod.ISECT_DTYPE))
        mrt_mod.intersect(sc, dev_ptr(d_rays), 80, len(rays), dev_ptr(d_out), precise=precise)
        got = from_dev(d_out, oracle_mod.ISECT_DTYPE)
        g = got[pos]
        assert len(set(g.tobytes()[k * 16:(k + 1) * 16] for k in range(len(g)))) == 1, precise
        prim = int(g["triangleIndex"][0])
        print(f"precise={precise}: prim {prim} t {_tbits(g['distance'][0])}")
        if precise:
            assert got.tobytes() == ref.tobytes()
            assert prim == VEC["ieee_hit"]["prim"] and _tbits(g["distance"][0]) == VEC["ieee_hit"]["t_bits"]
        else:
            assert prim in [h["prim"] for h in VEC["fast_build_hits"]]
    sc.close()
