"""The renderer's read-back entry points (mrt_renderer_read_*) as a group: which
fault wins when several apply, and that a resize leaves no derived plane
readable and no stale buffer behind.

The readers are called through mrt.lib() directly where the Python wrappers
cannot reach: they never pass a null or a short buffer."""
import ctypes

import numpy as np
import pytest

from camera_cases import camera

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_STATE = 0, -1, -5
W0, H0, L0 = 64, 48, 4
W1, H1 = 96, 64            # two tiles of 64x64


def _scene(mrt_mod, cache={}):
    if "s" not in cache:
        cache["s"] = mrt_mod.Scene("cornellbox")
    return cache["s"]


def status_of(mrt_mod, fn, *args):
    with pytest.raises(mrt_mod.MrtError) as e:
        fn(*args)
    return e.value.status


# name, elements per pixel (0: one per tile), and the message of a sufficient
# buffer on a renderer that has drawn and nothing else (None: the call succeeds)
STALE_SIZE = "has run at the renderer's current size"
READERS = [
    ("image", 4, None),
    ("moments", 4, None),
    ("denoised", 4, "no denoise " + STALE_SIZE),
    ("resolved", 4, "no resolve " + STALE_SIZE),
    ("variance", 1, "no mrt_renderer_denoise_variance " + STALE_SIZE),
    ("clamped", 4, "no firefly clamp " + STALE_SIZE),
    ("extra", 4, "no refine or draw_tiles " + STALE_SIZE),
    ("extra_moments", 4, "no refine or draw_tiles " + STALE_SIZE),
    ("tile_priority", 0, "no refine " + STALE_SIZE),
    ("tile_error", 0, "no error estimate " + STALE_SIZE),
    ("tile_list", 0, "no refine or draw_tiles " + STALE_SIZE),
]


def test_reader_error_precedence(gpu, mrt_mod):
    """Per reader: a null output is MRT_ERR_INVALID, a buffer one element short
    is MRT_ERR_INVALID, a sufficient one MRT_ERR_STATE with the entry point's own
    message — but for read_tile_list, which looks at the state before the
    capacity, and read_image / read_moments, which are never stale."""
    L = mrt_mod.lib()
    r = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=True, moments=True)
    r.resize(W1, H1)
    r.draw(2)
    T = r.tile_count()
    assert T == 2
    big = np.zeros(W1 * H1 * 4 + 8, np.float32)
    second = np.zeros(T + 8, np.uint32)
    out, out2 = ctypes.c_void_p(big.ctypes.data), ctypes.c_void_p(second.ctypes.data)
    n = ctypes.c_uint32()

    def call(name, ptr, count, ptr2=out2, pn=ctypes.byref(n)):
        fn = getattr(L, "mrt_renderer_read_" + name)
        if name == "clamped":
            rc = fn(r._h, ptr, count, pn)
        elif name == "tile_error":
            rc = fn(r._h, ptr, ptr2, count)
        elif name == "tile_list":
            rc = fn(r._h, ptr, count, pn)
        else:
            rc = fn(r._h, ptr, count)
        return rc, L.mrt_last_error().decode()

    for name, per_pixel, stale in READERS:
        need = W1 * H1 * per_pixel if per_pixel else T
        assert call(name, None, need) == (ERR_INVALID, "null argument"), name
        rc, msg = call(name, out, need - 1)
        if name == "tile_list":
            assert (rc, msg) == (ERR_STATE, stale), name
        else:
            assert (rc, msg) == (ERR_INVALID, "output buffer too small"), name
        rc, msg = call(name, out, need)
        if stale is None:
            assert rc == OK, (name, msg)
        else:
            assert (rc, msg) == (ERR_STATE, stale), name
    # the second outputs: required by read_tile_error and read_tile_list, optional for read_clamped
    assert call("tile_error", out, T, ptr2=None) == (ERR_INVALID, "null argument")
    assert call("tile_list", out, T, pn=None) == (ERR_INVALID, "null argument")
    assert call("clamped", out, W1 * H1 * 4, pn=None)[0] == ERR_STATE
    # the null check comes first everywhere
    assert call("variance", None, 0) == (ERR_INVALID, "null argument")
    assert L.mrt_renderer_read_image(None, out, big.size) == ERR_INVALID
    assert L.mrt_renderer_read_extra(None, out, big.size) == ERR_INVALID
    img, mom = r.read_image(), r.read_moments()
    assert np.isfinite(img).all() and img[..., :3].max() > 0 and (mom[..., 3] == 1.0).all()
    r.close()
    plain = mrt_mod.Renderer(_scene(mrt_mod), W0, H0, L0, precise=True)
    plain.draw(1)
    assert L.mrt_renderer_read_moments(plain._h, None, big.size) == ERR_INVALID
    assert L.mrt_renderer_read_moments(plain._h, out, W0 * H0 * 4 - 1) == ERR_INVALID
    assert L.mrt_renderer_read_moments(plain._h, out, W0 * H0 * 4) == ERR_STATE
    assert "without MRT_FLAG_MOMENTS" in L.mrt_last_error().decode()
    plain.close()


def test_resize_invalidates_every_derived_plane_once(gpu, mrt_mod):
    """After a resize no derived plane of the old size can be read or shown, and
    what is computed next equals, bitwise, what a renderer created at the new
    size computes.  (Nothing after a refine is compared: the refine schedule's
    extra-frame counter survives a resize by design.)"""
    sc, D = _scene(mrt_mod), camera(mrt_mod, "D")
    fp = mrt_mod.FireflyParams.default()

    def planes(r):
        r.draw(8)
        r.denoise_variance()
        s = r.error_estimate()
        return s, (r.read_denoised(), r.read_variance(), *r.read_clamped(), r.read_resolved(), *r.read_tile_error())

    r = mrt_mod.Renderer(sc, W0, H0, L0, precise=True, moments=True)
    r.set_firefly(fp)
    r.draw(8)
    r.denoise()
    r.move_camera(D)
    r.draw(8)
    r.denoise_variance()
    r.error_estimate()
    r.refine(1, 1)
    r.resolve()
    for read in (r.read_denoised, r.read_resolved, r.read_variance, r.read_clamped, r.read_extra, r.read_extra_moments,
                 r.read_tile_priority, r.read_tile_list, r.read_tile_error):
        read()                                   # every derived plane exists and is current
    r.resize(W1, H1)
    for read in (r.read_denoised, r.read_resolved, r.read_variance, r.read_clamped, r.read_extra, r.read_extra_moments,
                 r.read_tile_priority, r.read_tile_list, r.read_tile_error):
        assert status_of(mrt_mod, read) == ERR_STATE, read.__name__
    for flag in (mrt_mod.DISPLAY_DENOISED, mrt_mod.DISPLAY_RESOLVED):
        assert status_of(mrt_mod, r.display, flag) == ERR_STATE
        assert status_of(mrt_mod, r.display_enqueue, 0, flag) == ERR_STATE
    s_got, got = planes(r)
    assert r.camera.as_dict() == D.as_dict() and r.firefly.as_dict() == fp.as_dict()
    r.close()
    f = mrt_mod.Renderer(sc, W1, H1, L0, precise=True, moments=True)
    f.set_camera(D)
    f.set_firefly(fp)
    s_want, want = planes(f)
    f.close()
    assert s_got == s_want
    names = ("denoised", "variance", "clamped", "clamped count", "resolved", "tile error", "tile pixels")
    for name, g, w in zip(names, got, want):
        assert np.asarray(g).shape == np.asarray(w).shape, name
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes(), name
    assert got[0].shape == (H1, W1, 4) and got[5].shape == (2,) and np.isfinite(got[0]).all()
