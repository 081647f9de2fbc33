"""Generated rooms for the scene-detected shortcuts (occluder planes and the
second shadow tree, convex solids, camera-ray candidate lists): a seeded,
deterministic OBJ + MTL writer, so the detectors and the kernels' shortcut
branches are tested on geometry other than the shipped Cornell box.

The room is the shipped box's — x in [-1, 1], y in [0, 2], z in [-1, 1], open
at z = +1 — with diffuse walls (Ks 1 0 0) and a light emissive through Ka.
Blocks are six quads with outward windings and flat normals; coordinates are
written with %.9g, so every parser reads the same float32 values.

room(name, seed, directory) writes <name>-<seed>.obj / .mtl and returns a Room
recording what the detectors are expected to do with it (CASES)."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

F = np.float32

# name: (convex_solids expected, occluder tree expected)
CASES = {
    "plain-1": (1, True), "plain-2": (2, True), "plain-3": (3, True), "plain-4": (4, True),
    "plain-5": (0, True),       # more than 4 solids: no convex test, the tree stays
    "skew": (4, True),          # tops sheared by up to 0.05 per unit height
    "float": (2, True),         # one block at y0 = 0.3: all six faces kept
    "nobottom": (2, True),      # no bottom quads (the floor's plane stands in)
    "wall": (2, True),          # a side face in the left wall's (culled) plane
    "stacked": (2, True),       # a small block's bottom coplanar with a larger block's top
    "crossing": (2, True),      # two interpenetrating blocks
    "touching": (0, True),      # two blocks sharing corner positions: one component, not convex
    "smooth": (0, True),        # per-vertex radial normals
    "inward": (0, True),        # flat normals pointing into the block
    "wedge": (0, True),         # a triangular prism: 5 faces
    "underlight": (2, True),    # a block top 0.015 under the light
    "twolights": (3, True),     # two light quads: 4 light triangles
    "walllight": (2, True),     # a vertical light 0.01 in front of the back wall
    "plastic": (2, True),       # one block Ks 0 0 -1.5
    "glass": (2, True),         # one block Ks 0 0 1.5
}
DETECTING = [n for n, (c, _) in CASES.items() if c > 0]


def seeds(name):
    """The two seeds the tests use per case.  float's seed 1 is left to a test
    of its own: there the occluder tree comes out deeper than the main tree,
    so the library drops it (scene_api.cpp build_occluder_tree) and no shortcut is detected."""
    return (2, 3) if name == "float" else (1, 2)

MTL = """newmtl white
Kd 0.8 0.8 0.8
Ks 1.0 0.0 0.0

newmtl red
Kd 0.8 0.1 0.1
Ks 1.0 0.0 0.0

newmtl green
Kd 0.1 0.8 0.1
Ks 1.0 0.0 0.0

newmtl block
Kd 0.7 0.7 0.9
Ks 1.0 0.0 0.0

newmtl plastic
Kd 0.9 0.5 0.2
Ks 0.0 0.0 -1.5

newmtl glass
Kd 1 1 1
Ks 0.0 0.0 1.5

newmtl light
Kd 1 1 1
Ks 1.0 0.0 0.0
Ka 5 4 3
"""

LIGHT_Y = 1.985   # 0.015 under the ceiling


@dataclass
class Room:
    name: str
    seed: int
    path: str
    convex_solids: int
    occluder_tree: bool
    blocks: list   # each block's 8 corners [8, 3] (base 0-3, top 4-7), in file order

    @property
    def id(self) -> str:
        return f"{self.name}-{self.seed}"


class _Mesh:
    def __init__(self):
        self.v, self.n, self.groups, self.blocks = [], [], [], []

    def face(self, pts, normal, mtl):
        """A polygon (fan-triangulated by every parser) with one normal."""
        k = len(self.v)
        self.v.extend([tuple(float(F(c)) for c in p) for p in pts])
        self.n.append(tuple(float(F(c)) for c in normal))
        self.groups.append((mtl, [(k + i + 1, len(self.n)) for i in range(len(pts))]))

    def face_vn(self, pts, normals, mtl):
        """A polygon with one normal per corner."""
        k, m = len(self.v), len(self.n)
        self.v.extend([tuple(float(F(c)) for c in p) for p in pts])
        self.n.extend([tuple(float(F(c)) for c in q) for q in normals])
        self.groups.append((mtl, [(k + i + 1, m + i + 1) for i in range(len(pts))]))

    def write(self, path):
        base = os.path.splitext(os.path.basename(path))[0]
        with open(path, "w") as f:
            f.write(f"mtllib {base}.mtl\n")
            for p in self.v:
                f.write("v %.9g %.9g %.9g\n" % p)
            for q in self.n:
                f.write("vn %.9g %.9g %.9g\n" % q)
            for mtl, corners in self.groups:
                f.write(f"usemtl {mtl}\n")
                f.write("f " + " ".join(f"{v}//{n}" for v, n in corners) + "\n")
        with open(os.path.join(os.path.dirname(path), base + ".mtl"), "w") as f:
            f.write(MTL)


def _walls(m):
    m.face([(-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)], (0, 1, 0), "white")      # floor
    m.face([(-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)], (0, -1, 0), "white")     # ceiling
    m.face([(1, 0, -1), (1, 2, -1), (-1, 2, -1), (-1, 0, -1)], (0, 0, 1), "white")    # back wall
    m.face([(-1, 0, -1), (-1, 2, -1), (-1, 2, 1), (-1, 0, 1)], (1, 0, 0), "red")      # left wall
    m.face([(1, 0, 1), (1, 2, 1), (1, 2, -1), (1, 0, -1)], (-1, 0, 0), "green")       # right wall


def _ceiling_light(m, x0, x1, z0, z1):
    m.face([(x0, LIGHT_Y, z0), (x1, LIGHT_Y, z0), (x1, LIGHT_Y, z1), (x0, LIGHT_Y, z1)], (0, -1, 0), "light")


def _corners(cx, cz, a, b, angle, y0, h, shear=(0.0, 0.0)):
    """The 8 corners of a block: base rectangle (half sizes a, b, turned by
    `angle` about y, centred at (cx, cz)) at y0, top at y0 + h moved by
    shear * h (a parallelepiped).  Rounded to float32 here, so shared corners
    of two blocks are bit-equal."""
    c, s = np.cos(angle), np.sin(angle)
    base = [(cx + c * x - s * z, y0, cz + s * x + c * z) for x, z in ((-a, -b), (a, -b), (a, b), (-a, b))]
    top = [(x + shear[0] * h, y0 + h, z + shear[1] * h) for x, _, z in base]
    return np.array(base + top, F).astype(np.float64)


# corner indices of the six quads: bottom, top, four sides
_QUADS = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]


def _block(m, P, mtl="block", bottom=True, normals="flat"):
    """Six quads over the corners P [8, 3], each wound so that e1 x e2 points
    away from the block's centre.  normals: "flat" (the face's unit normal),
    "inward" (its negative) or "smooth" (per corner, from the centre)."""
    cen = P.mean(0)
    m.blocks.append(P)
    for k, q in enumerate(_QUADS):
        if k == 0 and not bottom:
            continue
        pts = P[list(q)]
        n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
        n /= np.linalg.norm(n)
        if n @ (pts[0] - cen) < 0:
            pts, n = pts[::-1], -n
        if normals == "smooth":
            rad = pts - cen
            m.face_vn(pts, rad / np.linalg.norm(rad, axis=1, keepdims=True), mtl)
        else:
            m.face(pts, n if normals == "flat" else -n, mtl)


def _wedge(m, cx, cz, a, b, h):
    """A triangular prism standing on the floor: 2 triangles, 3 quads."""
    base = np.array([(cx - a, 0, cz - b), (cx + a, 0, cz - b), (cx, 0, cz + b)], F).astype(np.float64)
    top = base + np.array([0, float(F(h)), 0])
    P = np.concatenate([base, top])
    cen = P.mean(0)
    for q in [(0, 1, 2), (3, 4, 5), (0, 1, 4, 3), (1, 2, 5, 4), (2, 0, 3, 5)]:
        pts = P[list(q)]
        n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
        n /= np.linalg.norm(n)
        if n @ (pts[0] - cen) < 0:
            pts, n = pts[::-1], -n
        m.face(pts, n, "block")


# block sites: 0.6 apart, a rotated base (half sizes <= 0.16) plus its shear stays in its cell
_SITES = [(x, z) for z in (-0.5, 0.25) for x in (-0.6, 0.0, 0.6)]


def _standing(rng, count, shear=0.0, avoid=()):
    """`count` blocks on distinct sites: (cx, cz, a, b, angle, y0, h, shear)."""
    sites = [s for s in rng.permutation(len(_SITES)) if s not in avoid][:count]
    out = []
    for s in sites:
        cx, cz = _SITES[s]
        cx, cz = cx + rng.uniform(-0.04, 0.04), cz + rng.uniform(-0.04, 0.04)
        sh = (rng.uniform(-shear, shear), rng.uniform(-shear, shear))
        out.append((cx, cz, rng.uniform(0.08, 0.16), rng.uniform(0.08, 0.16), rng.uniform(0, np.pi), 0.0,
                    rng.uniform(0.3, 1.3), sh))
    return out


def room(name: str, seed: int, directory: str) -> Room:
    """Write the named case for `seed` into `directory`; the same name and seed
    always give the same files."""
    if name not in CASES:
        raise KeyError(name)
    rng = np.random.default_rng([seed, sorted(CASES).index(name)])
    m = _Mesh()
    _walls(m)
    light = True
    if name.startswith("plain-"):
        for b in _standing(rng, int(name[6:])):
            _block(m, _corners(*b))
    elif name == "skew":
        for b in _standing(rng, 4, shear=0.05):
            _block(m, _corners(*b))
    elif name == "float":
        a, b = _standing(rng, 2)
        _block(m, _corners(*a))
        _block(m, _corners(*b[:5], 0.3, min(b[6], 0.9)))
    elif name == "nobottom":
        for b in _standing(rng, 2):
            _block(m, _corners(*b), bottom=False)
    elif name == "wall":
        (a,) = _standing(rng, 1, avoid=(0, 3))
        _block(m, _corners(*a))
        w = rng.uniform(0.1, 0.2)
        _block(m, _corners(-1.0 + w, rng.uniform(-0.5, 0.3), w, rng.uniform(0.1, 0.2), 0.0, 0.0, rng.uniform(0.4, 1.2)))
    elif name == "stacked":
        cx, cz, ang, h = rng.uniform(-0.3, 0.3), rng.uniform(-0.4, 0.2), rng.uniform(0, np.pi), rng.uniform(0.4, 0.8)
        big = _corners(cx, cz, 0.3, 0.25, ang, 0.0, h)
        _block(m, big)
        # the small block starts at the big one's top height (the float32 value: coplanar)
        _block(m, _corners(cx + rng.uniform(-0.08, 0.08), cz + rng.uniform(-0.08, 0.08), 0.12, 0.1,
                           rng.uniform(0, np.pi), float(big[4, 1]), rng.uniform(0.2, 0.5)))
    elif name == "crossing":
        cx, cz = rng.uniform(-0.3, 0.3), rng.uniform(-0.4, 0.2)
        _block(m, _corners(cx, cz, 0.3, 0.14, rng.uniform(0, np.pi), 0.0, rng.uniform(0.5, 0.9)))
        _block(m, _corners(cx + rng.uniform(-0.05, 0.05), cz + rng.uniform(-0.05, 0.05), 0.14, 0.3,
                           rng.uniform(0, np.pi), 0.0, rng.uniform(1.0, 1.3)))
    elif name == "touching":
        cx, cz, a, b, h = rng.uniform(-0.3, 0.1), rng.uniform(-0.4, 0.2), 0.15, 0.12, rng.uniform(0.4, 0.9)
        A = _corners(cx, cz, a, b, 0.0, 0.0, h)
        _block(m, A)
        # the neighbour takes A's +x face's four corner positions, bit for bit
        B = A.copy()
        B[[0, 3, 4, 7]] = A[[1, 2, 5, 6]]
        B[[1, 2, 5, 6]] = A[[1, 2, 5, 6]] + np.array([float(F(0.25)), 0, 0])
        _block(m, np.array(B, F).astype(np.float64))
    elif name in ("smooth", "inward"):
        a, b = _standing(rng, 2)
        _block(m, _corners(*a))
        _block(m, _corners(*b), normals=name)
    elif name == "wedge":
        (a,) = _standing(rng, 1, avoid=(1,))
        _block(m, _corners(*a))
        _wedge(m, 0.0 + rng.uniform(-0.04, 0.04), -0.5, 0.15, 0.12, rng.uniform(0.4, 1.0))
    elif name == "underlight":
        (a,) = _standing(rng, 1, avoid=(1, 4))
        _block(m, _corners(*a))
        _block(m, _corners(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.12, 0.1, rng.uniform(0, np.pi), 0.0,
                           LIGHT_Y - 0.015))
    elif name == "twolights":
        for b in _standing(rng, 3):
            _block(m, _corners(*b))
        _ceiling_light(m, -0.85, -0.05, -0.8, 0.7)
        _ceiling_light(m, 0.05, 0.85, -0.8, 0.7)
        light = False
    elif name == "walllight":
        for b in _standing(rng, 2):
            _block(m, _corners(*b))
        m.face([(-0.9, 0.4, -0.99), (0.9, 0.4, -0.99), (0.9, 1.9, -0.99), (-0.9, 1.9, -0.99)], (0, 0, 1), "light")
        light = False
    elif name in ("plastic", "glass"):
        a, b = _standing(rng, 2)
        _block(m, _corners(*a))
        _block(m, _corners(*b), mtl=name)
    if light:
        _ceiling_light(m, -0.8, 0.8, -0.8, 0.7)
    path = os.path.join(str(directory), f"{name}-{seed}.obj")
    m.write(path)
    return Room(name, seed, path, *CASES[name], m.blocks)
