"""CPU: the convex-occluder shadow decision (dev_shadow.h convex_occlusion,
occluders.h ConvexSet) against the brute-force leaf test, in float32.

On C2's scene every triangle of the light-free occluder tree lies on one of
two convex solids (the blocks).  A shadow ray through that tree is decided
per solid: the segment [o, o + t_T d] against the solid's face planes pushed
out by delta (Cyrus-Beck); a ray from a face of a solid with d . n >= 1e-3
(the face's own outward normal) skips that solid; otherwise the triangles of the face the
segment enters (or leaves) through are leaf-tested with the occlusion rule,
and a lane none of them certifies leaf-tests the solid's other faces (so no
lane walks the occluder tree).

The certificate and exhaustive sides are exact by construction (they are
the leaf test).  The "no solid occludes" side rests on a margin, so it is
checked here: over
>= 1 M adversarial shadow rays — origins on every occluder-tree-eligible
surface offset by 1e-4 along the normal as shade_hit does, light samples on
the light, and rays aimed at the blocks' edges and corners and grazing
their faces at 1e-3 ... 1e-7 — no ray classified "clear" has a block triangle
that the leaf test (tri_bary's float32 arithmetic, without and with one FMA
contraction pattern, and with the fast build's approximate reciprocals on top
of it: "rcp") accepts in [0, t_T].

The same certificates run on 20 generated rooms (tests/roomgen.py): 1 to 4
solids, sheared, floating, bottomless, on a wall's plane, stacked, crossing,
under the light, with two lights, a wall light and non-diffuse blocks."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import roomgen
from helpers import SEED

F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _dot(a, b, fma):
    if fma:
        return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F)))
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def _cross(a, b, fma):
    if fma:
        return np.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                         _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                         _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1).astype(F)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


ARITH = [False, True, "rcp"]   # the `fma` argument below: IEEE, FMA contraction, and FMA + approximate reciprocals
ARITH_IDS = ["ieee", "fma", "rcp"]


def _recip(x, fma):
    """1 / x in float32.  "rcp": the fast build's v_rcp_f32 (1 ulp): the
    correctly rounded reciprocal moved by -1, 0 or +1 ulp, chosen by a hash of
    the operand's bits — a pure function of the operand, as the hardware's
    result is, so two tests of one triangle by one ray see one reciprocal."""
    inv = (F(1) / x).astype(F)
    if fma != "rcp":
        return inv
    k = (np.ascontiguousarray(x, F).view(np.uint32) * np.uint32(0x9E3779B1)) >> np.uint32(30)   # 0..3; 0, 3: keep
    u = np.ascontiguousarray(inv).view(np.uint32)
    plain = ((u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)) & ((u & np.uint32(0x7FFFFFFF)) != 0)
    u = np.where(plain & (k == 1), u + np.uint32(1), np.where(plain & (k == 2), u - np.uint32(1), u)).astype(np.uint32)
    return u.view(F)


def _tri_bary(o, d, v0, v1, v2, fma):
    """dev_math.h tri_bary (+ the leaf test's validity), float32."""
    e1, e2 = (v1 - v0).astype(F), (v2 - v0).astype(F)
    p = _cross(d, e2, fma)
    det = _dot(e1, p, fma)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = _recip(det, fma)
        s = (o - v0).astype(F)
        b1 = (_dot(s, p, fma) * inv).astype(F)
        q = _cross(s, e1, fma)
        b2 = (_dot(d, q, fma) * inv).astype(F)
        t = (_dot(e2, q, fma) * inv).astype(F)
        ok = (det != 0) & (b1 >= 0) & (b1 <= 1) & (b2 >= 0) & ((b1 + b2).astype(F) <= 1)
    return ok, t


def _classify(o, d, tT, own, own_n, info, prims, target, fma, count=None):
    """dev_shadow.h convex_occlusion, float32: 1 occluded, 0 clear by the slabs
    or the own face, -1 left to the exhaustive test of a solid (not occluded).
    count, if given, collects how many (ray, solid) tests had no entry face
    (the segment starts inside the padded solid): all of them, and those
    against a solid other than the origin's own."""
    n = len(o)
    occluded = np.zeros(n, bool)
    undecided = np.zeros(n, bool)
    obb = np.array(info["convex_obb"], F)                 # [solid][16]
    pairs = np.array(info["convex_face_tris"], np.uint32)  # [solid][8]
    # the origin's own solid is skipped when d . n_face >= 1e-3 (its face's own normal, kConvexLeaveDot)
    own_skip = np.where((own != 0) & (_dot(own_n, d, fma) >= F(1e-3)), (own.astype(np.int64) - 1) >> 3, -1)
    for c in range(info["convex_solids"]):
        B = obb[c]
        t0 = np.zeros(n, F)
        t1 = tT.copy()
        fin = np.full(n, 8, np.uint32)
        fout = np.full(n, 8, np.uint32)
        for a in range(3):
            nv = np.broadcast_to(B[3 * a:3 * a + 3], d.shape)
            nd = _dot(nv, d, fma)
            no = _dot(nv, o, fma)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = _recip(nd, fma)
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
        leaves_own = own_skip == c
        cand = (t0 <= t1) & ~leaves_own & ~occluded
        if count is not None:
            count["empty_entry"] += int((cand & (fin == 8)).sum())
            count["empty_entry_other"] += int((cand & (fin == 8) & (((own.astype(np.int64) - 1) >> 3) != c)).sum())
        pp = np.concatenate([pairs[c], np.full(1, 0xFFFFFFFF, np.uint32)])
        pin, pout = pp[np.minimum(fin, 8)], pp[np.minimum(fout, 8)]
        pin = np.where(fin < 6, pin, 0xFFFFFFFF).astype(np.uint32)
        pout = np.where(fout < 6, pout, 0xFFFFFFFF).astype(np.uint32)

        def face(pair):
            hit = np.zeros(n, bool)
            for j in range(2):
                prim = (pair >> (16 * j)) & 0xFFFF
                valid = prim != 0xFFFF
                pi = np.where(valid, prim, 0)
                ok, t = _tri_bary(o, d, prims[pi, 0], prims[pi, 1], prims[pi, 2], fma)
                hit |= valid & ok & (pi != target) & (t >= 0) & (t <= tT) & ((t < tT) | (pi < target))
            return hit
        hit = face(np.where(pin != 0xFFFFFFFF, pin, pout))
        hit2 = face(pout)
        hit = hit | (~hit & (pin != 0xFFFFFFFF) & hit2)
        undecided |= cand & ~hit   # (the kernel then leaf-tests the solid's other faces)
        for k in range(6):
            hk = face(np.full(n, pairs[c, k], np.uint32))
            hit = hit | (~hit & (fin != k) & (fout != k) & hk)
        occluded |= cand & hit
    return np.where(occluded, 1, np.where(undecided, -1, 0))


def _solid_faces(info):
    """(own-face code c * 8 + face + 1 per primitive, the solids' primitives)."""
    pairs = np.array(info["convex_face_tris"], np.uint32)[:info["convex_solids"]]
    own, solid = {}, []
    for c in range(pairs.shape[0]):
        for k in range(6):
            for j in range(2):
                p = (int(pairs[c, k]) >> (16 * j)) & 0xFFFF
                if p != 0xFFFF:
                    own[p] = c * 8 + k + 1
                    solid.append(p)
    return own, sorted(solid)


def _face_normals(info, V, tri):
    """Per primitive: its solid face's outward unit normal (occluders.cpp: the
    face's first triangle's e1 x e2 in double, turned away from the solid's
    corner centroid, rounded to float32 — the shading record's n0.w..n2.w);
    zero off the solids."""
    pairs = np.array(info["convex_face_tris"], np.uint32)[:info["convex_solids"]]
    out = np.zeros((len(tri), 3), F)
    for c in range(pairs.shape[0]):
        ps = [(int(pairs[c, k]) >> (16 * j)) & 0xFFFF for k in range(6) for j in range(2)]
        ps = [p for p in ps if p != 0xFFFF]
        corners = np.unique(V[tri[ps]].reshape(-1, 3).astype(np.float64), axis=0)
        cen = corners.mean(0)
        for k in range(6):
            first = int(pairs[c, k]) & 0xFFFF
            if first == 0xFFFF:
                continue
            v = V[tri[first]].astype(np.float64)
            nr = np.cross(v[1] - v[0], v[2] - v[0])
            nr /= np.linalg.norm(nr)
            if nr @ cen - nr @ v[0] > 0:
                nr = -nr
            for j in range(2):
                p = (int(pairs[c, k]) >> (16 * j)) & 0xFFFF
                if p != 0xFFFF:
                    out[p] = nr.astype(F)
    return out


def _load(mrt_mod, obj):
    """(info, V, N, tri, export) of a scene as the library flattens it."""
    s = mrt_mod.Scene(obj, device=-1)
    e = s.export()
    info = dict(s.info)
    s.close()
    V = e["vertices"]["v"].astype(F)
    N = e["vertices"]["n"].astype(F)
    tri = e["references"]["tri"]
    return info, V, N, tri, e


@pytest.fixture(scope="module")
def box(mrt_mod):
    return _load(mrt_mod, "cornellbox")


# the generated rooms (tests/roomgen.py) the certificates run on: every
# detecting case at its first seed and five of them at a second: 20 scenes
ROOMS = [(n, roomgen.seeds(n)[0]) for n in roomgen.DETECTING] + \
        [(n, roomgen.seeds(n)[1]) for n in ("plain-3", "plain-4", "skew", "stacked", "crossing")]
ROOM_IDS = [f"{n}-{s}" for n, s in ROOMS]


@pytest.fixture(scope="module")
def rooms(mrt_mod, tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("rooms"), {}

    def get(name, seed):
        if (name, seed) not in cache:
            rm = roomgen.room(name, seed, d)
            cache[name, seed] = (rm, _load(mrt_mod, rm.path))
        return cache[name, seed]
    return get


def _rays(info, V, N, tri, e, rng, n, inside=False):
    """Adversarial shadow rays: origins on random surface points (offset
    1e-4 along the interpolated normal, shade_hit's sh.o), light samples on
    the light; half of them aimed at or grazing the blocks' edges, corners
    and faces.  inside: up to a tenth of the origins are moved to points of
    a solid's face that lie inside (or on a face coplanar with) ANOTHER solid's
    padded box, where there are any (stacked and crossing solids): segments
    that start inside a solid; and an aimed ray takes the light triangle it
    reaches as its target."""
    T = len(tri)
    lights = np.nonzero(e["references"]["lightTriangleIndex"] != 0xFFFFFFFF)[0]
    _, solid_tris = _solid_faces(info)
    # origins: uniform over the scene's triangles (weight 1 each) and biased to block faces near edges
    ot = rng.integers(0, T, n)
    ot[: n // 3] = rng.choice(solid_tris, n // 3)
    r1, r2 = rng.random(n).astype(F), rng.random(n).astype(F)
    edge = rng.random(n) < 0.5
    r1 = np.where(edge, F(1) - rng.random(n).astype(F) * F(1e-3) ** rng.integers(1, 3, n).astype(F), r1)
    sq = np.sqrt(r1).astype(F)
    w = np.stack([F(1) - sq, sq * (F(1) - r2), sq * r2], 1).astype(F)
    v = V[tri[ot]]
    nv = N[tri[ot]]
    hv = (v[:, 0] * w[:, :1] + v[:, 1] * w[:, 1:2] + v[:, 2] * w[:, 2:]).astype(F)
    hn = (nv[:, 0] * w[:, :1] + nv[:, 1] * w[:, 1:2] + nv[:, 2] * w[:, 2:]).astype(F)
    hn = (hn / np.sqrt((hn * hn).sum(1, keepdims=True))).astype(F)
    o = (hv + hn * F(1e-4)).astype(F)
    if inside:
        m = n // 10
        own_map, _ = _solid_faces(info)
        solid_of = np.full(T, -1)
        for p, code in own_map.items():
            solid_of[p] = (code - 1) >> 3
        ct = rng.choice(solid_tris, 16 * m)
        c1, c2 = np.sqrt(rng.random(16 * m)).astype(F), rng.random(16 * m).astype(F)
        cw = np.stack([F(1) - c1, c1 * (F(1) - c2), c1 * c2], 1).astype(F)
        cv, cn = V[tri[ct]], N[tri[ct]]
        ch = (cv[:, 0] * cw[:, :1] + cv[:, 1] * cw[:, 1:2] + cv[:, 2] * cw[:, 2:]).astype(F)
        cnn = (cn[:, 0] * cw[:, :1] + cn[:, 1] * cw[:, 1:2] + cn[:, 2] * cw[:, 2:]).astype(F)
        cnn = (cnn / np.sqrt((cnn * cnn).sum(1, keepdims=True))).astype(F)
        co = (ch + cnn * F(1e-4)).astype(F)
        within = np.zeros(16 * m, bool)
        for c in range(info["convex_solids"]):
            B = np.array(info["convex_obb"][c], np.float64)
            inc = solid_of[ct] != c
            for a in range(3):
                x = co.astype(np.float64) @ B[3 * a:3 * a + 3]
                inc &= (x >= B[9 + 2 * a]) & (x <= B[10 + 2 * a])
            within |= inc
        pick = np.nonzero(within)[0][:m]
        if len(pick):
            ot[n - len(pick):] = ct[pick]
            o[n - len(pick):] = co[pick]
    # targets: a random light triangle point
    lt = rng.choice(lights, n)
    a, b = rng.random(n).astype(F), rng.random(n).astype(F)
    sa = np.sqrt(a).astype(F)
    lw = np.stack([F(1) - sa, sa * (F(1) - b), sa * b], 1).astype(F)
    lv = V[tri[lt]]
    q = (lv[:, 0] * lw[:, :1] + lv[:, 1] * lw[:, 1:2] + lv[:, 2] * lw[:, 2:]).astype(F)
    # half the rays aim past a block edge / corner / face point instead, then on to
    # the light's plane (the target test decides whether they still reach it)
    aim = rng.random(n) < 0.5
    st = rng.choice(solid_tris, n)
    bv = V[tri[st]]
    k = rng.integers(0, 3, n)
    corner = bv[np.arange(n), k]
    nxt = bv[np.arange(n), (k + 1) % 3]
    s = rng.random(n).astype(F)
    pt = (corner + (nxt - corner) * s[:, None]).astype(F)
    jitter = (rng.standard_normal((n, 3)) * (F(10.0) ** -rng.integers(3, 8, n))[:, None]).astype(F)
    pt = (pt + jitter).astype(F)
    dq = (q - o).astype(F)
    dp = (pt - o).astype(F)
    d = np.where(aim[:, None], dp, dq).astype(F)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(F)
    if inside:
        # an aimed ray that reaches a light triangle takes that one as its target
        reach = np.zeros(n, bool)
        for L in lights:
            ok, t = _tri_bary(o, d, V[tri[L]][0], V[tri[L]][1], V[tri[L]][2], False)
            reach |= aim & ok & (t > 0)
            lt = np.where(aim & ok & (t > 0), L, lt)
        # one that reaches none is turned round: the line from its light point q
        # through the edge point is followed to the room's walls or floor (the
        # triangles off the solids and lights), and the ray starts there — a
        # shadow ray that grazes the edge on its way to the light
        redo = np.nonzero(aim & ~reach)[0]
        back = (pt[redo] - q[redo]).astype(F)
        back = (back / np.sqrt((back * back).sum(1, keepdims=True))).astype(F)
        best = np.full(len(redo), np.inf, F)
        wall = np.zeros(len(redo), np.int64)
        on_solid = set(solid_tris) | set(int(x) for x in lights)
        for w_ in (t_ for t_ in range(T) if t_ not in on_solid):
            ok, t = _tri_bary(q[redo], back, V[tri[w_]][0], V[tri[w_]][1], V[tri[w_]][2], False)
            near = ok & (t > F(1e-3)) & (t < best)
            best, wall = np.where(near, t, best), np.where(near, w_, wall)
        found = np.isfinite(best)
        redo, back, best, wall = redo[found], back[found], best[found], wall[found]
        wn = N[tri[wall]][:, 0]   # (walls and floor: one normal per face)
        o[redo] = ((q[redo] + back * best[:, None]).astype(F) + wn * F(1e-4)).astype(F)
        ot[redo] = wall
        dn = (pt[redo] - o[redo]).astype(F)
        d[redo] = (dn / np.sqrt((dn * dn).sum(1, keepdims=True))).astype(F)
    return o, d, ot, lt


def _check_clear(scene, fma, rng, rounds, n, inside=False):
    """The kernel model's "occluded" against the brute force over the solids'
    triangles on rounds x n adversarial rays of one scene; the counts."""
    info, V, N, tri, e = scene
    prims = V[tri]                                   # [T, 3, 3]
    planes = np.array(info["occluder_plane"][:info["occluder_planes"]], F)
    margin = F(info["occluder_margin"])
    stats = dict(rays=0, via_tree=0, clear=0, occluded=0, undecided=0, empty_entry=0, empty_entry_other=0)
    own_map, solid = _solid_faces(info)
    own_face = np.zeros(len(tri), np.uint32)
    for p, f in own_map.items():
        own_face[p] = f
    own_normal = _face_normals(info, V, tri)
    for _ in range(rounds):
        o, d, ot, lt = _rays(info, V, N, tri, e, rng, n, inside)
        # the target test (tri_test) gives t_T; rays missing the light are not queried
        okT, tT = _tri_bary(o, d, prims[lt, 0], prims[lt, 1], prims[lt, 2], fma)
        keep = okT & (tT >= F(1e-4))
        # shadow_root: inside every culled plane by the margin -> the occluder tree
        inside_planes = np.ones(n, bool)
        for P in planes:
            inside_planes &= (_dot(np.broadcast_to(P[:3], o.shape), o, fma) - P[3]) <= -margin
        keep &= inside_planes
        o, d, ot, lt, tT = o[keep], d[keep], ot[keep], lt[keep], tT[keep]
        cls = _classify(o, d, tT, own_face[ot], own_normal[ot], info, prims, lt, fma, stats)
        # brute force over the blocks' triangles: the occlusion rule
        occ = np.zeros(len(o), bool)
        for t in solid:
            ok, t_ = _tri_bary(o, d, prims[t, 0], prims[t, 1], prims[t, 2], fma)
            occ |= ok & (t != lt) & (t_ >= 0) & (t_ <= tT) & ((t_ < tT) | (t < lt))
        # the kernel's answer ("occluded" iff cls == 1) is the brute force's:
        # clear lanes by the margin, certified and exhaustively tested ones
        # (cls == -1: the first faces did not certify) by the leaf test itself
        bad = np.nonzero((cls == 1) != occ)[0]
        assert len(bad) == 0, (len(bad), cls[bad[:3]], o[bad[:3]], d[bad[:3]])
        stats["rays"] += n
        stats["via_tree"] += len(o)
        for name, v in (("clear", 0), ("occluded", 1), ("undecided", -1)):
            stats[name] += int((cls == v).sum())
    return stats


_ARITH_SEED = {False: 0, True: 1, "rcp": 2}
CLEAR_ROUNDS, CLEAR_RAYS = 2, 200_000   # per generated room and arithmetic


@pytest.mark.parametrize("fma", ARITH, ids=ARITH_IDS)
def test_convex_clear_rays_are_never_hit(mrt_mod, box, fma):
    info = box[0]
    assert info["convex_solids"] == 2
    assert len(_solid_faces(info)[1]) == 20   # the blocks' 5 faces x 2 triangles each (their bottoms are culled)
    stats = _check_clear(box, fma, np.random.default_rng(SEED + _ARITH_SEED[fma]), 14, 200_000)
    print(stats)
    assert stats["via_tree"] >= 1_000_000, stats
    # (adversarial rays: half aimed within 1e-3 ... 1e-7 of a block edge, so
    # far more of them are undecided — left to the exhaustive test — than in a render)
    assert stats["undecided"] <= 0.1 * stats["via_tree"]


def _each_arithmetic(fn):
    """fn(fma) for the three arithmetics, side by side (numpy releases the
    interpreter lock in its loops); the results in ARITH's order."""
    with ThreadPoolExecutor(len(ARITH)) as pool:
        return [f.result() for f in [pool.submit(fn, fma) for fma in ARITH]]


@pytest.mark.parametrize("name,seed", ROOMS, ids=ROOM_IDS)
def test_convex_clear_rays_are_never_hit_in_generated_rooms(rooms, name, seed):
    """The same certificate on the generated rooms: 1 to 4 solids, six-face
    and bottomless solids, a face on a wall's culled plane, stacked and
    crossing solids (a tenth of the origins inside another solid's padded
    box), four light triangles, a wall light.  400 k rays per scene and
    arithmetic (IEEE, FMA, FMA + approximate reciprocals); at least half reach
    the occluder tree, and at most a quarter are left to the exhaustive branch
    (measured: DESIGN.md 2.1e)."""
    rm, scene = rooms(name, seed)
    info = scene[0]
    assert info["convex_solids"] == rm.convex_solids and info["occluder_planes"] > 0

    def run(fma):
        rng = np.random.default_rng([SEED, _ARITH_SEED[fma], ROOMS.index((name, seed))])
        return _check_clear(scene, fma, rng, CLEAR_ROUNDS, CLEAR_RAYS, inside=True)
    for arith, stats in zip(ARITH_IDS, _each_arithmetic(run)):
        print(rm.id, arith, stats, "undecided share %.4f" % (stats["undecided"] / stats["via_tree"]),
              "via_tree share %.3f" % (stats["via_tree"] / stats["rays"]))
        assert stats["rays"] == 400_000
        assert stats["via_tree"] >= 0.5 * stats["rays"], stats
        assert stats["undecided"] <= 0.25 * stats["via_tree"], stats
        if name in ("stacked", "crossing"):
            assert stats["empty_entry_other"] > 1000, stats


def _check_grazing(scene, fma, rng, rounds, n):
    """(rays that hit their own solid, the largest d . n_face among them) over
    rounds x n grazing rays from the solids' faces."""
    info, V, N, tri, e = scene
    prims = V[tri]
    own_map, solid = _solid_faces(info)
    normals = _face_normals(info, V, tri)
    pairs = np.array(info["convex_face_tris"], np.uint32)
    worst, hits = -1.0, 0
    own_face = np.zeros(len(tri), np.int64)
    for p, f in own_map.items():
        own_face[p] = f
    for _ in range(rounds):
        ot = rng.choice(solid, n)
        r1, r2 = rng.random(n).astype(F), rng.random(n).astype(F)
        edge = rng.random(n) < 0.7
        r1 = np.where(edge, F(1) - rng.random(n).astype(F) * F(10.0) ** -rng.uniform(1, 6, n).astype(F), r1)
        sq = np.sqrt(r1).astype(F)
        w = np.stack([F(1) - sq, sq * (F(1) - r2), sq * r2], 1).astype(F)
        w = np.take_along_axis(w, rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1), 1)
        v, nv = V[tri[ot]], N[tri[ot]]
        hv = (v[:, 0] * w[:, :1] + v[:, 1] * w[:, 1:2] + v[:, 2] * w[:, 2:]).astype(F)
        hn = (nv[:, 0] * w[:, :1] + nv[:, 1] * w[:, 1:2] + nv[:, 2] * w[:, 2:]).astype(F)
        hn = (hn / np.sqrt((hn * hn).sum(1, keepdims=True))).astype(F)
        o = (hv + hn * F(1e-4)).astype(F)
        fn = normals[ot].astype(np.float64)
        tan = rng.standard_normal((n, 3))
        tan -= (tan * fn).sum(1, keepdims=True) * fn
        tan /= np.linalg.norm(tan, axis=1, keepdims=True)
        tilt = rng.choice([-1.0, 1.0], n) * 10.0 ** -rng.uniform(1, 8, n)
        d = (tan + tilt[:, None] * fn)
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
        nd = _dot(normals[ot], d, fma)
        c_own = (own_face[ot] - 1) >> 3
        hit = np.zeros(n, bool)
        for c in range(info["convex_solids"]):
            mine = c_own == c
            for k in range(6):
                for j in range(2):
                    p = (int(pairs[c, k]) >> (16 * j)) & 0xFFFF
                    if p == 0xFFFF:
                        continue
                    ok, t = _tri_bary(o, d, prims[p, 0], prims[p, 1], prims[p, 2], fma)
                    hit |= mine & ok & (t >= 0) & (t <= F(4.0))
        hits += int(hit.sum())
        if hit.any():
            worst = max(worst, float(nd[hit].max()))
    return hits, worst


@pytest.mark.parametrize("fma", ARITH, ids=ARITH_IDS)
def test_own_face_grazing_rays_never_hit_their_solid(mrt_mod, box, fma):
    """The own-face skip (d . n >= 1e-3 over the face's own normal,
    kConvexLeaveDot) on the rays it is most exposed to: origins on the blocks'
    faces (offset 1e-4 along the interpolated shading normal, as shade_hit),
    70 % of them within 1e-1 ... 1e-6 (barycentric) of an edge, directions
    tangent to the face tilted by +-1e-1 ... 1e-8 along its normal, segments as
    long as the scene (t_T = 4): no ray that hits its own solid (any triangle
    the leaf test accepts in [0, t_T]) comes within 10x of the threshold."""
    hits, worst = _check_grazing(box, fma, np.random.default_rng(SEED + 7 + _ARITH_SEED[fma]), 5, 200_000)
    print(dict(hits=hits, worst_dot=worst))
    assert hits > 10_000                 # the sample reaches its solid often (rays tilted into it)
    assert worst < 1e-4                  # 10x below kConvexLeaveDot = 1e-3


@pytest.mark.parametrize("name,seed", ROOMS, ids=ROOM_IDS)
def test_own_face_grazing_rays_never_hit_their_solid_in_generated_rooms(rooms, name, seed):
    """The same on the generated rooms' solids (rotated, sheared, floating,
    stacked, crossing), 200 k rays per scene and arithmetic, with the same
    bound; the sample reaches its solid as often as on the Cornell box (1 %)."""
    rm, scene = rooms(name, seed)

    def run(fma):
        rng = np.random.default_rng([SEED, 7, _ARITH_SEED[fma], ROOMS.index((name, seed))])
        return _check_grazing(scene, fma, rng, 1, 200_000)
    for arith, (hits, worst) in zip(ARITH_IDS, _each_arithmetic(run)):
        print(rm.id, arith, dict(hits=hits, worst_dot=worst))
        assert hits > 2_000
        assert worst < 1e-4                  # 10x below kConvexLeaveDot = 1e-3
