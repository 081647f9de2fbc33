"""GPU side of the movable camera: mrt_raygen_camera against the oracle
(default camera) and a float64 model of the definition (moved cameras), the
renderer with moved cameras against the oracle's stages replayed from those
camera rays, set_camera's reset / ordering guarantees, the candidate lists of a
moved camera against the traversal, and the CLI's camera options.

The oracle has no camera: tests/camera_cases.py replays its stages from given
camera rays (validated against OracleScene.render in test_camera_host.py)."""
import os
import subprocess

import numpy as np
import pytest

from camera_cases import CAMERAS, camera, model_rays, replay_render
from helpers import SEED, dev_ptr, from_dev, pixel_metrics, to_dev

pytestmark = pytest.mark.gpu

# Fast-build ray generation against the float64 model, cameras A-E at 97x61:
# the largest component error measured on an MI355X was 2.27e-7 (camera E's
# origins; directions 1.39e-7); the test asserts four times
# that, below the project's fast-build gate for distances (1e-4,
# test_gpu_parity.py).
FAST_RAYGEN_MEASURED = 2.27e-7
FAST_RAYGEN_BOUND = min(4 * FAST_RAYGEN_MEASURED, 1e-4)


def _scene(mrt_mod, name, cache={}):
    if name not in cache:
        cache[name] = mrt_mod.Scene(name)
    return cache[name]


def _oscene(oracle_mod, mrt_mod, name, cache={}):
    if name not in cache:
        cache[name] = oracle_mod.OracleScene(mrt_mod.scene_path(name))
    return cache[name]


def _gpu_rays(mrt_mod, oracle_mod, sc, cam, W, H, noise, precise=True):
    d_noise = to_dev(noise)
    d_rays = to_dev(np.zeros(W * H, oracle_mod.RAY_DTYPE))
    mrt_mod.raygen(sc, W, H, dev_ptr(d_noise), dev_ptr(d_rays), precise=precise, camera=cam)
    return from_dev(d_rays, oracle_mod.RAY_DTYPE)   # (no .copy(): it leaves a padded record's padding undefined)


@pytest.mark.parametrize("W,H", [(64, 48), (257, 131)])
def test_raygen_default_camera_bitexact(gpu, mrt_mod, oracle_mod, W, H):
    sc = _scene(mrt_mod, "cornellbox")
    noise = oracle_mod.noise_table(SEED, 3)
    got = _gpu_rays(mrt_mod, oracle_mod, sc, mrt_mod.Camera.default(), W, H, noise)
    assert got.tobytes() == oracle_mod.raygen(W, H, noise).tobytes()


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_raygen_matches_model(gpu, mrt_mod, oracle_mod, name):
    W, H = 97, 61
    sc, cam = _scene(mrt_mod, "cornellbox"), camera(mrt_mod, name)
    noise = oracle_mod.noise_table(SEED, 5)
    o_ref, d_ref = model_rays(cam, W, H, noise)
    # precise: fewer than 20 roundings on operands of magnitude max(1, s, focus)
    scale = max(1.0, float(cam.tan_half_fov), float(cam.focus_distance))
    for precise in (True, False):
        rays = _gpu_rays(mrt_mod, oracle_mod, sc, cam, W, H, noise, precise=precise)
        eo = np.abs(rays["origin"].astype(np.float64) - o_ref).max()
        ed = np.abs(rays["direction"].astype(np.float64) - d_ref).max()
        unit = np.abs(np.linalg.norm(rays["direction"].astype(np.float64), axis=1) - 1.0).max()
        print(f"camera {name} {'precise' if precise else 'fast'}: origin err {eo:.3g}, direction err {ed:.3g}, "
              f"| |d| - 1 | {unit:.3g}")
        assert np.all(rays["maxDistance"] == np.inf) and np.all(rays["throughput"] == 1.0)
        if precise:
            assert max(eo, ed) <= 4e-6 * scale
            assert unit <= 4e-7
        else:
            assert max(eo, ed) <= FAST_RAYGEN_BOUND
    if cam.lens_radius > 0:   # the lens moves the origins, inside its disc
        off = np.linalg.norm(rays["origin"].astype(np.float64) - np.array(list(cam.origin)), axis=1)
        assert off.max() <= cam.lens_radius * (1 + 1e-5) and off.max() > 0.5 * cam.lens_radius


def _render(mrt_mod, sc, W, H, L, frames, precise, cam=None, shard=(0, 1)):
    r = mrt_mod.Renderer(sc, W, H, L, precise=precise, shard_rank=shard[0], shard_count=shard[1])
    if cam is not None:
        r.set_camera(cam)
    r.draw(frames)
    img, st = r.read_image(), r.stats()
    r.close()
    return img, st


def _replay(mrt_mod, oracle_mod, scene, cam, W, H, L, frames, cache={}):
    """The oracle's image from the precise build's camera rays (computed once per case)."""
    key = (scene, bytes(cam), W, H, L, frames)
    if key not in cache:
        sc, osc = _scene(mrt_mod, scene), _oscene(oracle_mod, mrt_mod, scene)
        cache[key] = replay_render(
            oracle_mod, osc, W, H, L, frames,
            lambda f: _gpu_rays(mrt_mod, oracle_mod, sc, cam, W, H, oracle_mod.noise_table(SEED, f)))
    return cache[key]


def _check_against_replay(mrt_mod, oracle_mod, scene, cam, W, H, L, frames, precise, kernel):
    sc = _scene(mrt_mod, scene)
    ref = _replay(mrt_mod, oracle_mod, scene, cam, W, H, L, frames)
    img, st = _render(mrt_mod, sc, W, H, L, frames, precise, cam)
    rel, rmse, same = pixel_metrics(img, ref)
    print(f"{scene} {W}x{H} L={L} f={frames} kernel {st['kernel']}: bit-identical {same:.5f}, "
          f"rel<=1e-4 {np.mean(rel <= 1e-4):.5f}, rmse {rmse:.2e}")
    assert st["kernel"] == kernel
    assert st["paths"] == W * H * frames
    assert np.all(img[..., 3] == 1.0)
    assert ref[..., :3].max() > 0
    if precise:   # the gates of test_render_parity_precise
        assert np.mean(rel <= 1e-4) >= 0.999
        assert rmse <= 1e-3
    else:         # the fast build's gate
        assert np.mean(rel <= 1e-2) >= 0.99


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_render_matches_replay(gpu, mrt_mod, oracle_mod, name):
    _check_against_replay(mrt_mod, oracle_mod, "cornellbox", camera(mrt_mod, name), 64, 48, 4, 3, True, 2)


@pytest.mark.parametrize("kernel,code", [("path", 1), ("wave", 0)])
@pytest.mark.parametrize("name", ["A", "E"])
def test_render_matches_replay_other_kernels(gpu, mrt_mod, oracle_mod, monkeypatch, name, kernel, code):
    monkeypatch.setenv("MRT_KERNEL", kernel)
    if kernel == "wave":   # one launch per bounce (bounce_kernel), not the streaming wavefront
        monkeypatch.setenv("MRT_STREAM", "0")
    _check_against_replay(mrt_mod, oracle_mod, "cornellbox", camera(mrt_mod, name), 64, 48, 4, 3, True, code)


def test_render_matches_replay_water(gpu, mrt_mod, oracle_mod):
    """A scene traversed from global memory: the path kernel by default."""
    _check_against_replay(mrt_mod, oracle_mod, "CornellBox-Water-plastic", camera(mrt_mod, "W"), 48, 36, 8, 2, True, 1)


@pytest.mark.parametrize("name", ["A", "E"])
def test_render_matches_replay_fast(gpu, mrt_mod, oracle_mod, name):
    _check_against_replay(mrt_mod, oracle_mod, "cornellbox", camera(mrt_mod, name), 64, 48, 4, 3, False, 2)


@pytest.mark.parametrize("precise", [True, False])
def test_set_default_camera_changes_nothing(gpu, mrt_mod, precise):
    sc = _scene(mrt_mod, "cornellbox")
    a, sa = _render(mrt_mod, sc, 97, 61, 4, 3, precise)
    b, sb = _render(mrt_mod, sc, 97, 61, 4, 3, precise, mrt_mod.Camera.default())
    assert a.tobytes() == b.tobytes()
    assert sa["primary_blocks"] == sb["primary_blocks"] > 0
    assert sa["active_ray_bounces"] == sb["active_ray_bounces"]


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("W,H", [(97, 61), (256, 144)])
def test_moved_camera_lists_equal_traversal(gpu, mrt_mod, monkeypatch, W, H, precise):
    sc, cam = _scene(mrt_mod, "cornellbox"), camera(mrt_mod, "A")
    monkeypatch.setenv("MRT_PRIMARY", "1")
    a, sa = _render(mrt_mod, sc, W, H, 4, 3, precise, cam)
    e, se = _render(mrt_mod, sc, W, H, 4, 3, precise, camera(mrt_mod, "E"))
    monkeypatch.setenv("MRT_PRIMARY", "0")
    b, sb = _render(mrt_mod, sc, W, H, 4, 3, precise, cam)
    assert sa["primary_blocks"] > 0 and sa["kernel"] == 2 and sb["primary_blocks"] == 0
    assert se["primary_blocks"] == 0   # a thin lens has no single origin: no lists
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    if precise:
        assert sa["active_ray_bounces"] == sb["active_ray_bounces"]
        assert a.tobytes() == b.tobytes()
    else:   # test_primary_lists_bitwise's fast gate
        assert abs(sa["active_ray_bounces"] - sb["active_ray_bounces"]) <= sb["active_ray_bounces"] // 1000
        rel = np.abs(a - b).max(-1) / (np.abs(b).max(-1) + 1e-3)
        assert np.mean(rel <= 1e-2) >= 0.999


@pytest.mark.parametrize("env,W,H,shard", [
    ({}, 97, 61, (0, 1)),
    ({"MRT_INFLIGHT": "3", "MRT_BATCH": "2"}, 97, 61, (0, 1)),
    ({}, 300, 200, (1, 3)),                                       # a tile share: two render streams
])
def test_set_camera_with_draws_in_flight(gpu, mrt_mod, monkeypatch, env, W, H, shard):
    """draw(3) with camera A, set_camera(B), draw(3), no sync in between: the
    image is that of a fresh renderer with camera B (B's upload is awaited on
    every render stream).  And draw(3) with camera A, then set_camera(B) alone
    with no sync: the image, which keeps its content until the next frame, is
    camera A's — the draws in flight did not read B's block or lists."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, A, B = _scene(mrt_mod, "cornellbox"), camera(mrt_mod, "A"), camera(mrt_mod, "B")
    fresh, sf = _render(mrt_mod, sc, W, H, 4, 3, True, B, shard)
    r = mrt_mod.Renderer(sc, W, H, 4, precise=True, shard_rank=shard[0], shard_count=shard[1])
    r.set_camera(A)
    r.draw(3)
    r.set_camera(B)
    assert bytes(r.camera) == bytes(B)
    r.draw(3)
    img, st = r.read_image(), r.stats()
    r.close()
    assert st["frame_index"] == 3
    assert st["paths"] == 2 * sf["paths"]          # the cumulative counters are kept
    assert img.tobytes() == fresh.tobytes()
    fresh_a, _ = _render(mrt_mod, sc, W, H, 4, 3, True, A, shard)
    r = mrt_mod.Renderer(sc, W, H, 4, precise=True, shard_rank=shard[0], shard_count=shard[1])
    r.set_camera(A)
    r.draw(3)
    r.set_camera(B)
    kept, st2 = r.read_image(), r.stats()
    r.close()
    assert st2["frame_index"] == 0
    assert kept.tobytes() == fresh_a.tobytes() and kept.tobytes() != fresh.tobytes()
    if env:
        assert st["inflight"] == 3


def test_cli_camera_options(gpu, mrt_mod, tmp_path):
    """mrt_render --eye/--target/--fov renders what the binding renders with
    the same look_at camera."""
    exe = os.path.join(os.path.dirname(mrt_mod.LIB_PATH), "..", "bin", "mrt_render")
    eye, target, up, fov, _, _ = CAMERAS["A"]
    out = tmp_path / "cam.pfm"
    p = subprocess.run([exe, "--scene", "cornellbox", "--w", "64", "--h", "48", "--spp", "2", "--L", "4", "--precise",
                        "--eye", ",".join(map(repr, eye)), "--target", ",".join(map(repr, target)),
                        "--fov", repr(fov), "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with open(out, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        img = np.frombuffer(f.read(), "<f4").reshape(h, w, 3)
    ours, _ = _render(mrt_mod, _scene(mrt_mod, "cornellbox"), 64, 48, 4, 2, True, camera(mrt_mod, "A"))
    plain, _ = _render(mrt_mod, _scene(mrt_mod, "cornellbox"), 64, 48, 4, 2, True)
    assert (w, h) == (64, 48)
    assert img.tobytes() == np.ascontiguousarray(ours[..., :3]).tobytes()
    assert img.tobytes() != np.ascontiguousarray(plain[..., :3]).tobytes()
