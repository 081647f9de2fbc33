"""CPU: the shadow query's face order (metal-renderer_amd/csrc/shadow_plan.h,
dev_shadow.h convex_occlusion) changes no decision.

1. The plan header, exhaustively (tools/shadow_plan_model.cpp compiles the text
   the kernels compile): every set of crossed solids out of 1 ... 4, every
   own-face skip, every entry and exit face code (8 = none included) and every
   pattern of hits; a lane's sequence of (solid, face) tests is the per-solid
   loop's — entry, exit, rest, each once, ending only at a hit — and so is its
   result.  Cap: 0 mismatches.
2. The decisions: a numpy restatement of the new order (slabs for every solid
   first, then one pass over each lane's first crossed solid's entry face, then
   the rest for the lanes that pass left open) against
   test_convex_occluders._classify on that file's adversarial rays — the
   Cornell box and the rooms plain-1, plain-4, stacked, crossing and skew, in
   IEEE, FMA and FMA + approximate-reciprocal arithmetic.  Cap: 0 disagreements.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import roomgen
import test_convex_occluders as tco
from helpers import SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-renderer_amd", "csrc")
F = np.float32


def test_plan_order_is_the_loops_exhaustively(tmp_path):
    exe = str(tmp_path / "shadow_plan_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC,
                    os.path.join(ROOT, "tools", "shadow_plan_model.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    cases, tests, mismatches, invariants = (int(re.search(rf"\b{n} (\d+)", r.stdout).group(1))
                                            for n in ("cases", "tests", "mismatches", "invariants"))
    assert r.returncode == 0 and mismatches == 0 and invariants == 0
    # 4 solids alone: 15 non-empty sets, 5 skips, 43 face-code pairs and 64 hit patterns for a solid of the set
    assert cases >= 15 * 5 * 43 * 64 and tests > cases


# ---- the plan in numpy (shadow_plan.h, word for word) ----
HAS, LATER = 1 << 10, 12


def _plan_add(plan, c, crossed, fin, fout):
    first = fin | (fout << 4) | (c << 8) | HAS
    later = plan | ((1 << LATER) << c)
    return np.where(crossed, np.where((plan & HAS) != 0, later, first), plan)


def _next_face(fin, fout, todo):
    ctz = np.zeros_like(todo)
    for k in range(5, -1, -1):
        ctz = np.where((todo >> k) & 1 != 0, k, ctz)
    return np.where((todo >> fin) & 1 != 0, fin, np.where((todo >> fout) & 1 != 0, fout, ctz))


def _merged(o, d, tT, own, own_n, info, prims, target, fma, count):
    """dev_shadow.h convex_occlusion in the new order, float32: occluded or not.
    count collects the face tests of the one pass and of the rest."""
    n = len(o)
    obb = np.array(info["convex_obb"], F)
    pairs = np.array(info["convex_face_tris"], np.uint32)
    solids = info["convex_solids"]
    # the staged table: 8 words per solid, faces 6 and 7 "no triangles"
    table = np.full(8 * max(solids, 1), 0xFFFFFFFF, np.uint32)
    for c in range(solids):
        table[8 * c:8 * c + 6] = pairs[c, :6]
    own_skip = np.where((own != 0) & (tco._dot(own_n, d, fma) >= F(1e-3)), (own.astype(np.int64) - 1) >> 3, -1)

    def slabs(c):
        B = obb[c]
        t0, t1 = np.zeros(n, F), tT.copy()
        fin, fout = np.full(n, 8, np.int64), np.full(n, 8, np.int64)
        for a in range(3):
            nv = np.broadcast_to(B[3 * a:3 * a + 3], d.shape)
            nd, no = tco._dot(nv, d, fma), tco._dot(nv, o, fma)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = tco._recip(nd, fma)
                tlo = ((B[9 + 2 * a] - no) * inv).astype(F)
                thi = ((B[10 + 2 * a] - no) * inv).astype(F)
            pos = ~np.signbit(nd)
            tn, tf = np.where(pos, tlo, thi), np.where(pos, thi, tlo)
            with np.errstate(invalid="ignore"):
                i_, o_ = tn > t0, tf < t1
            t0 = np.where(i_, tn, t0)
            fin = np.where(i_, np.where(pos, 2 * a, 2 * a + 1), fin)
            t1 = np.where(o_, tf, t1)
            fout = np.where(o_, np.where(pos, 2 * a + 1, 2 * a), fout)
        with np.errstate(invalid="ignore"):
            return t0 <= t1, fin, fout

    def face(at, lanes):
        """the leaf test of table[at]'s two triangles, for `lanes` only"""
        hit = np.zeros(n, bool)
        idx = np.nonzero(lanes)[0]
        if len(idx) == 0:
            return hit
        pair = table[at[idx]]
        for j in range(2):
            prim = (pair >> (16 * j)) & 0xFFFF
            valid = prim != 0xFFFF
            pi = np.where(valid, prim, 0)
            ok, t = tco._tri_bary(o[idx], d[idx], prims[pi, 0], prims[pi, 1], prims[pi, 2], fma)
            tg, tt = target[idx], tT[idx]
            hit[idx] |= valid & ok & (pi != tg) & (t >= 0) & (t <= tt) & ((t < tt) | (pi < tg))
        return hit

    plan = np.zeros(n, np.int64)
    kept = []
    for c in range(solids):
        crosses, fin, fout = slabs(c)
        kept.append((fin, fout))
        plan = _plan_add(plan, c, crosses & (own_skip != c), fin, fout)
    has = (plan & HAS) != 0
    p_fin, p_fout, p_solid = plan & 15, (plan >> 4) & 15, (plan >> 8) & 3
    first_face = np.where(p_fin != 8, p_fin, p_fout)
    occluded = face(p_solid * 8 + np.minimum(first_face, 7), has)
    count["pass"] += int(has.sum())
    more = has & ~occluded
    crossed = np.where(more, ((plan >> LATER) & 15) | (1 << p_solid), 0)
    for c in range(solids):
        fin, fout = kept[c]   # (the kernel computes the slabs again: the same words)
        todo = np.where(p_solid == c, 0x3F & ~(1 << first_face), 0x3F)
        hit = np.zeros(n, bool)
        mine = ((crossed >> c) & 1 != 0) & ~occluded
        while True:
            act = mine & (todo != 0) & ~hit
            if not act.any():
                break
            k = _next_face(fin, fout, todo)
            assert ((todo[act] >> k[act]) & 1 == 1).all() and (k[act] < 6).all()
            todo = np.where(act, todo & ~(1 << k), todo)
            hit |= face(c * 8 + np.minimum(k, 7), act)
            count["rest"] += int(act.sum())
        occluded |= hit
    return occluded


SCENES = ["cornellbox", "plain-1", "plain-4", "stacked", "crossing", "skew"]
RAYS = 150_000


@pytest.fixture(scope="module")
def scenes(mrt_mod, tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("shadow_plan"), {}

    def get(name):
        if name not in cache:
            cache[name] = tco._load(mrt_mod, "cornellbox" if name == "cornellbox"
                                    else roomgen.room(name, roomgen.seeds(name)[0], d).path)
        return cache[name]
    return get


@pytest.mark.parametrize("fma", tco.ARITH, ids=tco.ARITH_IDS)
@pytest.mark.parametrize("name", SCENES)
def test_new_order_decides_as_the_loop(scenes, name, fma):
    info, V, N, tri, e = scene = scenes(name)
    assert info["convex_solids"] == (2 if name == "cornellbox" else roomgen.CASES[name][0])
    prims = V[tri]
    rng = np.random.default_rng([SEED, 21, tco._ARITH_SEED[fma], SCENES.index(name)])
    own_map, _ = tco._solid_faces(info)
    own_face = np.zeros(len(tri), np.uint32)
    for p, f in own_map.items():
        own_face[p] = f
    own_normal = tco._face_normals(info, V, tri)
    o, d, ot, lt = tco._rays(info, V, N, tri, e, rng, RAYS, inside=name != "cornellbox")
    okT, tT = tco._tri_bary(o, d, prims[lt, 0], prims[lt, 1], prims[lt, 2], fma)
    keep = okT & (tT >= F(1e-4))   # (every ray that reaches its light: the query does not depend on the tree choice)
    o, d, ot, lt, tT = o[keep], d[keep], ot[keep], lt[keep], tT[keep]
    cls = tco._classify(o, d, tT, own_face[ot], own_normal[ot], info, prims, lt, fma)
    count = dict(**{"pass": 0}, rest=0)
    occ = _merged(o, d, tT, own_face[ot], own_normal[ot], info, prims, lt, fma, count)
    bad = np.nonzero((cls == 1) != occ)[0]
    print(f"{name} {fma}: rays {len(o)}, occluded {int(occ.sum())}, left to the rest {int((cls == -1).sum())}, "
          f"face tests: one pass {count['pass']}, rest {count['rest']}, disagreements {len(bad)}")
    assert len(o) >= RAYS // 3 and occ.sum() > 1000 and (cls == -1).sum() > 100
    assert len(bad) == 0, (len(bad), o[bad[:3]], d[bad[:3]])
