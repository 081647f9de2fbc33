#!/usr/bin/env python3
"""The convex shadow query's divergent passes per wave call, modelled on the
CPU: how many face passes a wave pays in the per-solid
loop (dev_shadow.h convex_occlusion_loop: one entry-face pass per solid that
any lane crosses) and with the plan (convex_occlusion: one pass for every
lane's first crossed solid), and how often the exit face and the exhaustive
rest run.

The rays are the oracle's shadow rays of C2's scene (cornellbox, L = 4), FRAMES
frames at W x H; the decisions are tests/test_convex_occluders._classify's
arithmetic (own-face rule: the face's own normal, d . n >= 1e-3) in the FMA
form.  Waves: at bounce 0 the 8 x 8 pixel blocks of the camera waves; at the
deeper bounces, whose queue levels mix pixels, LANES shadow lanes per call (the
stream kernel's average, tools/lane_stats.py shadow_phase_util), once in
pixel-block order and once in random order — the two ends the real queue order
lies between.

usage: tools/convex_branch_stats.py [scene] [W H FRAMES LANES]
"""
import os
import sys

import numpy as np


def _root():
    """The source tree this file lies in (the directory holding metal-renderer_amd/ and tests/)."""
    d = os.path.dirname(os.path.abspath(__file__))
    while not (os.path.isdir(os.path.join(d, "metal-renderer_amd")) and os.path.isdir(os.path.join(d, "tests"))):
        up = os.path.dirname(d)
        if up == d:
            raise SystemExit("convex_branch_stats.py: no source tree above " + os.path.abspath(__file__))
        d = up
    return d


ROOT = _root()
for sub in ("metal-renderer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))
import mrt      # noqa: E402
import oracle   # noqa: E402
from helpers import SEED   # noqa: E402
import test_convex_occluders as T   # noqa: E402

F = np.float32
FMA = True


def shadow_rays(osc, W, H, L, frames):
    """Per bounce: (pixel, origin, direction, target, origin primitive) of the oracle's shadow rays."""
    recs = {}
    pix = np.arange(W * H)
    for f in range(frames):
        rays = oracle.raygen(W, H, oracle.noise_table(SEED, f))
        for i in range(L):
            noise = oracle.noise_table(SEED, oracle.noise_frame_for(f, i))
            isect = osc.intersect_bvh(rays, threads=8)
            srays = np.zeros(len(rays), oracle.SRAY_DTYPE)
            osc.shade(W, H, f, L, noise, isect, rays, srays)
            ok = srays["maxDistance"] >= 0
            s = srays[ok]
            recs.setdefault(i, []).append((pix[ok] + f * W * H, s["origin"].astype(F), s["direction"].astype(F),
                                           s["targetIndex"].astype(np.int64), isect["triangleIndex"][ok].astype(np.int64)))
            sis = osc.intersect_bvh(srays, threads=8)
            oracle.resolve(sis, rays, srays)
    return {b: [np.concatenate([r[k] for r in v]) for k in range(5)] for b, v in recs.items()}


def classify(info, prims, own_face, own_normal, o, d, lt, org):
    """Per solid, per ray: crossed and not skipped, and which face test decides (as _classify, FMA form)."""
    n = len(o)
    okT, tT = T._tri_bary(o, d, prims[lt, 0], prims[lt, 1], prims[lt, 2], FMA)
    planes = np.array(info["occluder_plane"][:info["occluder_planes"]], F)
    inside = np.ones(n, bool)
    for P in planes:
        inside &= (T._dot(np.broadcast_to(P[:3], o.shape), o, FMA) - P[3]) <= -F(info["occluder_margin"])
    q = okT & (tT >= F(1e-4)) & inside   # the rays whose query goes to the convex test
    obb = np.array(info["convex_obb"], F)
    pairs = np.array(info["convex_face_tris"], np.uint32)
    own, own_n = own_face[org], own_normal[org]
    own_skip = np.where((own != 0) & (T._dot(own_n, d, FMA) >= F(1e-3)), (own.astype(np.int64) - 1) >> 3, -1)
    per = []
    for c in range(info["convex_solids"]):
        B = obb[c]
        t0, t1 = np.zeros(n, F), tT.copy()
        fin, fout = np.full(n, 8), np.full(n, 8)
        for a in range(3):
            nv = np.broadcast_to(B[3 * a:3 * a + 3], d.shape)
            nd, no = T._dot(nv, d, FMA), T._dot(nv, o, FMA)
            with np.errstate(all="ignore"):
                inv = T._recip(nd, FMA)
                tlo, thi = ((B[9 + 2 * a] - no) * inv).astype(F), ((B[10 + 2 * a] - no) * inv).astype(F)
            pos = ~np.signbit(nd)
            tn, tf = np.where(pos, tlo, thi), np.where(pos, thi, tlo)
            with np.errstate(invalid="ignore"):
                i_, o_ = tn > t0, tf < t1
            t0, fin = np.where(i_, tn, t0), np.where(i_, np.where(pos, 2 * a, 2 * a + 1), fin)
            t1, fout = np.where(o_, tf, t1), np.where(o_, np.where(pos, 2 * a + 1, 2 * a), fout)
        with np.errstate(invalid="ignore"):
            cand = q & (t0 <= t1) & (own_skip != c)
        pp = np.concatenate([pairs[c], np.full(3, 0xFFFFFFFF, np.uint32)])
        pin = np.where(fin < 6, pp[fin], 0xFFFFFFFF).astype(np.uint32)
        pout = np.where(fout < 6, pp[fout], 0xFFFFFFFF).astype(np.uint32)

        def face(pair):
            hit = np.zeros(n, bool)
            for j in range(2):
                prim = (pair >> (16 * j)) & 0xFFFF
                valid = prim != 0xFFFF
                pi = np.where(valid, prim, 0)
                ok, t = T._tri_bary(o, d, prims[pi, 0], prims[pi, 1], prims[pi, 2], FMA)
                hit |= valid & ok & (pi != lt) & (t >= 0) & (t <= tT) & ((t < tT) | (pi < lt))
            return hit
        h1 = face(np.where(pin != 0xFFFFFFFF, pin, pout))
        h2 = face(pout) & (pin != 0xFFFFFFFF)
        rest = np.zeros(n, bool)
        for k in range(6):
            rest |= (fin != k) & (fout != k) & face(np.full(n, pairs[c, k], np.uint32))
        per.append(dict(cand=cand, h1=h1, h2=h2, rest=rest, has_in=pin != 0xFFFFFFFF))
    return q, per


def wave_table(q, per, groups):
    """Per wave call (a row of `groups`: indices of its lanes, -1 = none): the passes of both forms."""
    valid = groups >= 0
    g = np.where(valid, groups, 0)

    def any_(mask):
        return (mask[g] & valid).any(1)
    calls = any_(q)
    n = len(q)
    occluded = np.zeros(n, bool)
    entry_now = np.zeros(len(groups))
    exit_ = np.zeros(len(groups))
    fallback = np.zeros(len(groups))
    first_done = np.zeros(n, bool)     # the lane has had its first crossed solid
    first_hit = np.zeros(n, bool)
    crossing = np.zeros(n, bool)
    for s in per:   # the per-solid loop
        live = s["cand"] & ~occluded
        entry_now += any_(live)
        need2 = live & ~s["h1"] & s["has_in"]
        exit_ += any_(need2)
        fb = live & ~s["h1"] & ~(need2 & s["h2"])
        fallback += any_(fb)
        occluded |= live & (s["h1"] | (need2 & s["h2"]) | (fb & s["rest"]))
        first = s["cand"] & ~first_done
        first_hit |= first & s["h1"]
        first_done |= s["cand"]
        crossing |= s["cand"]
    merged = any_(crossing)                       # the one pass
    rest_merged = any_(crossing & ~first_hit)     # a lane neither occluded nor done: the rest runs
    k = max(1, int(calls.sum()))
    lanes = (q[g] & valid).sum(1)[calls].mean() if calls.any() else 0.0
    cross = (crossing[g] & valid).sum(1)[calls].mean() if calls.any() else 0.0
    return dict(calls=int(calls.sum()), lanes=lanes, crossing=cross, entry_now=entry_now.sum() / k,
                merged=merged.sum() / k, exit=exit_.sum() / k, fallback=fallback.sum() / k,
                rest_merged=rest_merged.sum() / k)


def chunks(order, size):
    n = (len(order) + size - 1) // size
    out = np.full(n * size, -1, np.int64)
    out[:len(order)] = order
    return out.reshape(n, size)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cornellbox"
    W, H, frames, lanes = (int(x) for x in sys.argv[2:6]) if len(sys.argv) > 5 else (480, 272, 3, 44)
    L = 4
    sc = mrt.Scene(name, device=-1)
    info, e = dict(sc.info), sc.export()
    sc.close()
    osc = oracle.OracleScene.from_arrays(e["vertices"], e["references"], e["materials"])
    V, R = e["vertices"]["v"].astype(F), e["references"]["tri"]
    prims = V[R]
    own_map, _ = T._solid_faces(info)
    own_face = np.zeros(len(R), np.uint32)
    for p, f in own_map.items():
        own_face[p] = f
    own_normal = T._face_normals(info, V, R)
    print(f"{name} {W}x{H}, {frames} frames, L = {L}, {info['convex_solids']} solids; passes per shadow wave call")
    print("| bounce | waves | calls | crossing lanes per call | entry-face passes now | merged | exit-face passes | "
          "exhaustive fallback | rest runs (merged) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for b, (px, o, d, lt, org) in sorted(shadow_rays(osc, W, H, L, frames).items()):
        if len(o) == 0:
            continue
        q, per = classify(info, prims, own_face, own_normal, o, d, lt, org)
        fr, p = px // (W * H), px % (W * H)
        blk = (fr * ((H + 7) // 8) + (p // W) // 8) * ((W + 7) // 8) + (p % W) // 8
        order = np.argsort(blk, kind="stable")
        if b == 0:   # camera waves: a wave is a pixel block, whatever number of its lanes carries a shadow ray
            ids = np.unique(blk[order], return_inverse=True)[1]
            rows = np.full((ids.max() + 1, 64), -1, np.int64)
            slot = np.arange(len(order)) - np.searchsorted(ids, ids)
            rows[ids, slot] = order
            forms = [("8x8 blocks", rows)]
        else:
            qi = order[q[order]]
            forms = [(f"{lanes} lanes, block order", chunks(qi, lanes)),
                     (f"{lanes} lanes, random", chunks(np.random.default_rng(1).permutation(qi), lanes))]
        for what, groups in forms:
            t = wave_table(q, per, groups)
            print(f"| {b} | {what} | {t['calls']} | {t['crossing']:.1f} of {t['lanes']:.0f} | {t['entry_now']:.2f} | "
                  f"{t['merged']:.2f} | {t['exit']:.2f} | {t['fallback']:.2f} | {t['rest_merged']:.2f} |")


if __name__ == "__main__":
    main()
