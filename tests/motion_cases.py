"""Scene pairs shared by the moving-geometry tests (include/mrt.h
mrt_guides_motion, mrt_renderer_move_scene): two poses of one mesh, made here
from the shipped cornellbox.
  (a) cornellbox against a copy in which every vertex used by the shortBox
      faces is translated by SHIFT;
  (b) cornellbox + 512 procedural triangles, seed 1 against seed 2 (the same
      topology, another surface);
  (c) the same with 1 << 20 triangles under the device PLOC builder, whose tree
      needs the spill variant of the traversal stack (tests/test_gpu_guides.py)."""
from __future__ import annotations

import os

import numpy as np

SHIFT = (0.15, 0.0, 0.1)
BLOCK = "shortBox"
CENTRE = np.full(64 * 64 * 4, 0.5, np.float32)   # the noise table of the pixel-centre ray


def _groups(lines):
    """[(usemtl name, first line, one past the last line)] of the OBJ's face groups."""
    out, name, start = [], None, None
    for i, line in enumerate(lines):
        if line.startswith("g "):
            if name is not None:
                out.append((name, start, i))
            name, start = None, i
        elif line.startswith("usemtl ") and start is not None:
            name = line.split()[1]
    if name is not None:
        out.append((name, start, len(lines)))
    return out


def _lines(mrt_mod):
    with open(mrt_mod.scene_path("cornellbox")) as f:
        return f.read().splitlines()


def _write(directory, name, lines):
    path = os.path.join(str(directory), name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def mtl_path(mrt_mod):
    return mrt_mod.scene_path("cornellbox")[:-4] + ".mtl"


def moved_obj(mrt_mod, directory, shift=SHIFT, name="cornellbox_moved.obj"):
    """cornellbox with the vertices of the BLOCK faces translated by `shift`
    (load it with mtl_override = mtl_path())."""
    lines = _lines(mrt_mod)
    _, lo, hi = next(g for g in _groups(lines) if g[0] == BLOCK)
    used = {int(corner.split("/")[0]) for line in lines[lo:hi] if line.startswith("f ") for corner in line.split()[1:]}
    k = 0
    for i, line in enumerate(lines):
        if line.startswith("v "):
            k += 1
            if k in used:
                x, y, z = (float(t) for t in line.split()[1:4])
                lines[i] = f"v  {x + shift[0]:.5f} {y + shift[1]:.5f} {z + shift[2]:.5f}"
    assert len(used) == 8
    return _write(directory, name, lines)


def exchanged_obj(mrt_mod, directory, first="floor", second=BLOCK, name="cornellbox_exchanged.obj"):
    """cornellbox with the face groups `first` and `second` exchanged: the same
    triangles and materials, in another primitive order.  (Every vertex line
    first, then the groups: a face may only name vertices above it.)"""
    head, groups = [], []
    for line in _lines(mrt_mod):
        if line.startswith("g "):
            groups.append([line])
        elif line.startswith(("usemtl ", "f ", "s ")) and groups:
            groups[-1].append(line)
        else:
            head.append(line)
    names = [next(l.split()[1] for l in g if l.startswith("usemtl ")) for g in groups]
    a, b = names.index(first), names.index(second)
    groups[a], groups[b] = groups[b], groups[a]
    return _write(directory, name, head + [l for g in groups for l in g])


def _arrays(scene):
    """(vertices, references) of an mrt.Scene.export() dict or an OracleScene"""
    return (scene["vertices"], scene["references"]) if isinstance(scene, dict) else (scene.vertices, scene.references)


def moved_prims(a, b):
    """The primitives whose vertex positions differ between two poses."""
    (Va, Ra), (Vb, Rb) = _arrays(a), _arrays(b)
    assert np.array_equal(Ra["tri"], Rb["tri"])
    pa, pb = Va["v"][Ra["tri"].astype(np.int64)], Vb["v"][Rb["tri"].astype(np.int64)]
    return np.flatnonzero((pa != pb).any(axis=(1, 2)))
