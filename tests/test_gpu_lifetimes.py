"""GPU: the lifetimes of what a renderer owns on the host side (csrc/hip_handles.h: streams, events,
pinned and device memory released by their members, after the waits of ~mrt_renderer).  What can
go wrong on the device is a handle released while work still reads it, or released twice, or one
that was only lent (the caller's stream, the caller's image) released at all.  Cornell box, 64x64
unless stated; every comparison is bitwise."""
import numpy as np
import pytest

from helpers import dev_ptr, from_dev, to_dev

pytestmark = pytest.mark.gpu

L = 4
SIZES = [(64, 64), (192, 128), (64, 64)]


@pytest.fixture(scope="module")
def box(mrt_mod):
    return mrt_mod.Scene("cornellbox")


def _fresh(mrt_mod, box, W, H):
    """What a new renderer shows after draw(2): (image, blit of it)"""
    r = mrt_mod.Renderer(box, W, H, L, moments=True)
    r.draw(2)
    r.display_enqueue(0)
    out = r.read_image().tobytes(), r.display_map(0).tobytes()
    r.close()
    return out


@pytest.fixture(scope="module")
def fresh(gpu, mrt_mod, box):
    return {size: _fresh(mrt_mod, box, *size) for size in set(SIZES)}


def _four_frames(mrt_mod, box):
    r = mrt_mod.Renderer(box, 64, 64, L, moments=True)
    for _ in range(4):
        r.draw_frame()
    img = r.read_image().tobytes()
    r.close()
    return img


def test_destroy_with_work_in_flight(gpu, mrt_mod, box):
    """Eight renderers closed at once behind unsynchronised draws and a use of everything made at
    its first use (camera generations, the variance filter's planes, the refine draws' schedule,
    list and event, a display slot): close waits for the work, then releases; a renderer made
    afterwards renders what one made before did."""
    before = _four_frames(mrt_mod, box)
    cam = mrt_mod.Camera.look_at((0.0, 1.5, 0.3), (0.0, 0.3, -0.5), (0.0, 1.0, 0.0), 100.0)
    for _ in range(8):
        r = mrt_mod.Renderer(box, 64, 64, L, moments=True)
        for _ in range(3):
            r.draw_frame()
        r.set_camera(cam)
        r.draw_frame()
        r.denoise_variance()
        r.refine(1, 1)
        r.display_enqueue(0)
        r.close()
    assert _four_frames(mrt_mod, box) == before


def test_resize_up_and_down(gpu, mrt_mod, box, fresh):
    """The pinned buffers only grow (draw counters, tile-list staging, camera staging, display
    slot): back at the small size they are larger than the frame, and nothing of the large frame
    shows.  At each size the renderer equals a new one of that size."""
    r = mrt_mod.Renderer(box, *SIZES[0], L, moments=True)
    for k, (W, H) in enumerate(SIZES):
        if k:
            r.resize(W, H)
        r.draw(2)
        r.display_enqueue(0)
        shown = r.display_map(0)
        assert shown.shape == (H, W, 4)
        r.draw_tiles([0], 1)
        image = r.read_image()
        extra = r.read_extra()
        assert (image.tobytes(), shown.tobytes()) == fresh[(W, H)], (k, W, H)
        # the listed tile got its frame, no other pixel did
        count = extra[..., 3]
        assert count.sum() == 64 * 64 and np.count_nonzero(count) == 64 * 64, (k, W, H)
        assert r.refine_stats()["paths"] == (k + 1) * 64 * 64
    r.close()


def test_external_stream_and_image_are_not_released(gpu, mrt_mod, box, fresh):
    """A renderer on the caller's stream and image only borrows them: after its close the stream
    still carries its owner's draws and the image still holds what was drawn."""
    W, H = 64, 64
    owner = mrt_mod.Renderer(box, W, H, L, moments=True)
    d_img = to_dev(np.zeros((H, W, 4), np.float32))
    guest = mrt_mod.Renderer(box, W, H, L, stream=owner.stream(), image_ptr=dev_ptr(d_img))
    assert guest.stream() == owner.stream() and guest.image_ptr() == dev_ptr(d_img)
    guest.draw(2)
    guest.close()
    owner.draw(2)
    assert owner.read_image().tobytes() == fresh[(W, H)][0]
    assert from_dev(d_img, np.float32).tobytes() == fresh[(W, H)][0]
    owner.close()
