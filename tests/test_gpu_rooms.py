"""GPU: the scene-detected shortcuts (occluder tree, convex solids, camera-ray
candidate lists) on generated rooms (tests/roomgen.py) instead of the shipped
Cornell box: 1 to 5 blocks, sheared, floating, bottomless, stacked, crossing,
against a wall, just under the light, two lights, a light on the back wall, a
plastic and a glass block — and three rooms whose solids must not be detected.

a. every shortcut on equals every shortcut off, in each kernel and build;
b. the render equals the oracle's, which parses and flattens the OBJ itself
   and has none of the shortcuts;
c. a moved camera: lists on equal lists off, and the precise build equals the
   oracle's stages replayed from the GPU's own camera rays.

All at 96 x 64 (97 x 61 for the moved cameras), L = 4, 3 frames: milliseconds
per render, under a second per oracle render."""
import numpy as np
import pytest

import roomgen
from camera_cases import replay_render
from helpers import SEED, dev_ptr, from_dev, pixel_metrics, to_dev

pytestmark = pytest.mark.gpu

W, H, L, FRAMES = 96, 64, 4, 3
DETECTED = ["plain-3", "skew", "float", "stacked", "crossing", "wall", "twolights", "plastic",
            "nobottom", "underlight", "walllight", "glass"]
REFUSED = ["plain-5", "smooth", "touching"]
CASES = DETECTED + REFUSED
KERNELS = ["stream", "bounce", "path"]


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("gpu_rooms"), {}

    def get(name):
        if name not in cache:
            cache[name] = roomgen.room(name, roomgen.seeds(name)[0], d)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """The oracle's render of a room (computed once, shared, never written to)."""
    cache = {}

    def get(rm):
        if rm.id not in cache:
            img, A = oracle_mod.OracleScene(rm.path).render(W, H, L, SEED, FRAMES, threads=8)
            img.setflags(write=False)
            cache[rm.id] = (img, A)
        return cache[rm.id]
    return get


def _select(monkeypatch, kernel):
    monkeypatch.setenv("MRT_STREAM", "0" if kernel == "bounce" else "1")
    if kernel == "path":
        monkeypatch.setenv("MRT_KERNEL", "path")


def _render(mrt_mod, monkeypatch, path, precise, tree=True, convex=True, primary=True, size=(W, H), cam=None):
    """(image, stats, info) of a fresh scene and renderer under the given switches."""
    monkeypatch.setenv("MRT_CONVEX", "1" if convex else "0")
    monkeypatch.setenv("MRT_PRIMARY", "1" if primary else "0")
    s = mrt_mod.Scene(path, occluder_tree=tree)
    info = dict(s.info)
    r = mrt_mod.Renderer(s, size[0], size[1], L, precise=precise)
    if cam is not None:
        r.set_camera(cam)
    r.draw(FRAMES)
    img, st = r.read_image(), r.stats()
    r.close()
    s.close()
    return img, st, info


def _fast_gate(a, na, b, nb, what):
    """test_primary_lists_bitwise's fast gate; the bit-identical share is printed."""
    rel = np.abs(a - b).max(-1) / (np.abs(b).max(-1) + 1e-3)
    same = (a.view(np.uint32) == b.view(np.uint32)).all(-1).mean()
    print(f"{what}: bit-identical {same:.5f}, rel<=1e-2 {np.mean(rel <= 1e-2):.5f}, rays {na} vs {nb}")
    assert abs(na - nb) <= nb // 1000
    assert np.mean(rel <= 1e-2) >= 0.999


@pytest.mark.parametrize("build", ["precise", "fast"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", CASES)
def test_shortcuts_on_equal_shortcuts_off(gpu, mrt_mod, monkeypatch, room, name, kernel, build):
    """Everything on (the default), the convex test alone off (the occluder
    tree walked on a tree that is not the Cornell box's), and everything off
    (no occluder tree, no convex test, no candidate lists)."""
    rm, precise = room(name), build == "precise"
    _select(monkeypatch, kernel)
    a, sa, ia = _render(mrt_mod, monkeypatch, rm.path, precise)
    c, sc, ic = _render(mrt_mod, monkeypatch, rm.path, precise, convex=False)
    b, sb, ib = _render(mrt_mod, monkeypatch, rm.path, precise, tree=False, convex=False, primary=False)
    # the shortcuts were really active, and really off
    assert ia["convex_solids"] == rm.convex_solids and (rm.convex_solids == 0) == (name in REFUSED)
    assert ia["occluder_planes"] > 0 and ic["occluder_planes"] > 0 and ic["convex_solids"] == 0
    assert ib["occluder_planes"] == 0 and ib["convex_solids"] == 0 and sb["primary_blocks"] == 0
    if kernel == "path":   # the path kernel builds no lists (test_path_kernel_builds_no_lists)
        assert sa["kernel"] == 1 and sa["primary_blocks"] == 0
    else:
        assert sa["primary_blocks"] > 0
        if kernel == "stream":
            assert sa["kernel"] == 2
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    na, nc, nb = (s["active_ray_bounces"] for s in (sa, sc, sb))
    if precise:
        assert a.tobytes() == c.tobytes() and na == nc
        assert a.tobytes() == b.tobytes() and na == nb
    else:
        _fast_gate(a, na, c, nc, f"{rm.id} {kernel} fast, on vs convex off")
        _fast_gate(a, na, b, nb, f"{rm.id} {kernel} fast, on vs all off")


@pytest.mark.parametrize("build", ["precise", "fast"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", CASES)
def test_rooms_match_oracle(gpu, mrt_mod, monkeypatch, room, reference, name, kernel, build):
    """Precise build: every pixel bit-identical to the oracle's and the same
    active ray-bounce count (test_c3_full_size_matches_oracle's standard);
    fast build: test_render_parity_fast's gate."""
    rm = room(name)
    ref, A = reference(rm)
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    _select(monkeypatch, kernel)
    img, st, info = _render(mrt_mod, monkeypatch, rm.path, build == "precise")
    assert info["convex_solids"] == rm.convex_solids
    rel, rmse, same = pixel_metrics(img, ref)
    print(f"{rm.id} {kernel} {build}: solids {info['convex_solids']}, planes {info['occluder_planes']}, "
          f"lists {st['primary_blocks']}, bit-identical {same:.5f}, rel<=1e-2 {np.mean(rel <= 1e-2):.5f}, "
          f"rmse {rmse:.2e}, A {st['active_ray_bounces']} vs {A}")
    assert st["paths"] == W * H * FRAMES
    if build == "precise":
        assert same == 1.0 and st["active_ray_bounces"] == A
    else:
        assert np.mean(rel <= 1e-2) >= 0.99


def _cameras(mrt_mod, rm):
    """Two pinhole cameras: one inside the room, wide, whose camera plane cuts
    the walls' triangles; one low, 0.06 off a top corner of the first block,
    looking along its top towards the opposite corner."""
    P = rm.blocks[0]
    out = P[4] - P[4:].mean(0)
    eye = P[4] + 0.06 * out / np.linalg.norm(out) + np.array([0.0, 0.03, 0.0])
    target = P[6] - np.array([0.0, 0.1, 0.0])
    return {"inside": mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0),
            "edge": mrt_mod.Camera.look_at(tuple(eye), tuple(target), (0.0, 1.0, 0.0), 70.0)}


@pytest.mark.parametrize("build", ["precise", "fast"])
@pytest.mark.parametrize("cam", ["inside", "edge"])
@pytest.mark.parametrize("name", ["plain-3", "stacked"])
def test_moved_camera_in_rooms(gpu, mrt_mod, oracle_mod, monkeypatch, room, name, cam, build):
    """Lists on against lists off as test_moved_camera_lists_equal_traversal,
    and the precise build against the oracle's stages replayed from the GPU's
    own camera rays (test_gpu_camera's _check_against_replay).

    The low camera's plane cuts more than 12 triangles (floor, ceiling, side
    walls, the blocks' bottoms in the floor's plane, other blocks): with the
    default cap build_primary_lists refuses (more than `cap` triangles that
    every block must list) and every block traverses — asserted — so its lists
    are built with MRT_PRIMARY_CAP=24 (tools/primary_check.cpp: all 104 blocks
    listed, 0 violations)."""
    rm, size, precise = room(name), (97, 61), build == "precise"
    camera = _cameras(mrt_mod, rm)[cam]
    if cam == "edge":
        a0, s0, _ = _render(mrt_mod, monkeypatch, rm.path, precise, size=size, cam=camera)
        assert s0["primary_blocks"] == 0 and s0["kernel"] == 2
        monkeypatch.setenv("MRT_PRIMARY_CAP", "24")
    a, sa, _ = _render(mrt_mod, monkeypatch, rm.path, precise, size=size, cam=camera)
    b, sb, _ = _render(mrt_mod, monkeypatch, rm.path, precise, primary=False, size=size, cam=camera)
    assert sa["primary_blocks"] > 0 and sa["kernel"] == 2 and sb["primary_blocks"] == 0
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    na, nb = sa["active_ray_bounces"], sb["active_ray_bounces"]
    if not precise:
        _fast_gate(a, na, b, nb, f"{rm.id} camera {cam} fast, lists on vs off")
        return
    assert na == nb and a.tobytes() == b.tobytes()
    if cam == "edge":
        assert a0.tobytes() == b.tobytes() and s0["active_ray_bounces"] == nb
    sc, osc = mrt_mod.Scene(rm.path), oracle_mod.OracleScene(rm.path)

    def rays(f):
        d_noise = to_dev(oracle_mod.noise_table(SEED, f))
        d_rays = to_dev(np.zeros(size[0] * size[1], oracle_mod.RAY_DTYPE))
        mrt_mod.raygen(sc, size[0], size[1], dev_ptr(d_noise), dev_ptr(d_rays), precise=True, camera=camera)
        return from_dev(d_rays, oracle_mod.RAY_DTYPE)
    ref = replay_render(oracle_mod, osc, size[0], size[1], L, FRAMES, rays)
    sc.close()
    rel, rmse, same = pixel_metrics(a, ref)
    print(f"{rm.id} camera {cam}: lists {sa['primary_blocks']}, bit-identical {same:.5f}, "
          f"rel<=1e-4 {np.mean(rel <= 1e-4):.5f}, rmse {rmse:.2e}")
    assert ref[..., :3].max() > 0
    assert np.mean(rel <= 1e-4) >= 0.999 and rmse <= 1e-3   # the gates of test_render_parity_precise
