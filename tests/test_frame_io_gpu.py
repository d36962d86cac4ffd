"""The shared host plumbing of the frame stages (csrc/frame_io.h): staging a strided host image, fetching the
result, the one way into a tracker slot and the kernel timers -- every stage bitwise against its numpy oracle, on
shapes small enough for each route (integer / general / convert-only, byte / dword / run loads) to be one launch.
Every host source is a view into a wider array: its row stride is row bytes + 5."""
import ctypes as C

import numpy as np
import pytest

import equalize_oracle as eo
import ingest_oracle as io
import mask_oracle as mo
import resize_general_oracle as rgo
import warp_oracle as wo

pytestmark = pytest.mark.gpu

TW, TH = 64, 32  # the tracker of the slot tests


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def strided(W, H, bpp, seed):
    """(H, W, bpp) u8 noise ((H, W) for bpp 1) as a view into rows 5 bytes longer"""
    wide = np.random.default_rng(seed).integers(0, 256, (H, W * bpp + 5), dtype=np.uint8)
    v = wide[:, :W * bpp]
    v = v if bpp == 1 else v.reshape(H, W, bpp)
    assert v.strides[0] == W * bpp + 5
    return v


def strided_mask(W, H, seed):
    """a usable-region mask with excluded rectangles and isolated excluded pixels, strided as above"""
    rng = np.random.default_rng(seed)
    wide = np.full((H, W + 5), 255, np.uint8)
    m = wide[:, :W]
    m[H // 4:H // 2, W // 5:W // 3] = 0
    m[rng.integers(0, H, 6), rng.integers(0, W, 6)] = 0
    m[:, W - 2:] = 0
    return m


@pytest.mark.parametrize("W,H,dW,dH", [(37, 10, 9, 5),    # general path, staged pitch 48
                                       (32, 8, 8, 2)])    # factor 4, pitch 32: the factor-4 kernel's layout
def test_grey_round_trip(ctx, W, H, dW, dH):
    src = strided(W, H, 1, 1)
    want = rgo.resize_area_any(np.ascontiguousarray(src), dW, dH)
    np.testing.assert_array_equal(ctx.ingest(src, io.GRAY8, 0, dW, dH), want)
    np.testing.assert_array_equal(ctx.resize_area_any(src, dW, dH), want)
    if W % dW == 0 and H % dH == 0:
        np.testing.assert_array_equal(ctx.resize_area(src, dW, dH), want)


@pytest.mark.parametrize("fmt,W,H,dW,dH,rules", [
    (io.BGR8, 38, 12, 19, 6, (io.CVTCOLOR, io.IMREAD)),    # integer, run-of-2 kernel
    (io.BGR8, 38, 12, 9, 5, (io.CVTCOLOR, io.IMREAD)),     # general, 8-tap run kernel
    (io.BGRA8, 38, 12, 38, 12, (io.CVTCOLOR,)),            # convert only, dword source after staging
    (io.YUYV, 38, 12, 19, 6, (io.CVTCOLOR,)),              # integer, byte source
])
def test_packed_round_trip(ctx, fmt, W, H, dW, dH, rules):
    src = strided(W, H, io.BPP[fmt], 2)
    for rule in rules:
        np.testing.assert_array_equal(ctx.ingest(src, fmt, rule, dW, dH), io.ingest(src, fmt, rule, dW, dH))


def test_equalize_round_trip(vio, ctx):
    src = strided(35, 18, 1, 3)
    src //= 2  # in place: still the strided view; a narrow grey range, so equalisation has work to do
    src += 40
    np.testing.assert_array_equal(ctx.equalize(src, vio.equalize_params(vio.VIO_EQ_HIST)), eo.equalize_hist(src))
    np.testing.assert_array_equal(ctx.equalize(src, vio.equalize_params(vio.VIO_EQ_CLAHE, 2, 2, 3.0)),
                                  eo.clahe(src, 2, 2, 3.0))


def test_mask_round_trip(vio, ctx):
    m = strided_mask(37, 11, 4)
    np.testing.assert_array_equal(ctx.mask_build(m, 9, 5, vio.mask_params(1)), mo.build(m, 9, 5, 1))


def rotated_maps(sW, sH, dW, dH):
    mx, my = wo.map_erp(sW, sH, dW, dH, wo.rot_y(0.3))
    return mx.astype(np.float32), my.astype(np.float32)


def test_warp_round_trip(ctx):
    src = strided(21, 9, 3, 5)
    mx, my = rotated_maps(21, 9, 16, 8)
    w = ctx.warp_create(mx, my, 21, 9, wo.X_WRAP, wo.Y_REPLICATE)
    try:
        for rule in (io.CVTCOLOR, io.IMREAD):
            np.testing.assert_array_equal(w.apply(src, io.BGR8, rule),
                                          wo.remap(src, io.BGR8, rule, mx, my, wo.X_WRAP, wo.Y_REPLICATE))
    finally:
        w.close()


# ---- one way into a tracker slot ----

def slot(vio, ctx, torch, t, k):
    """the slot's frame, through a 1:1 device copy"""
    ptr, pitch = C.c_void_p(), C.c_int()
    ctx.check(vio.lib().erp_tracker_device_frame(t.h, k, C.byref(ptr), C.byref(pitch)), "erp_tracker_device_frame")
    dev = torch.zeros((t.H, t.W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.resize_area_any_device(ptr.value, t.W, t.H, pitch.value, 1, dev.data_ptr(), t.W, t.H, t.W)
    ctx.resize_kernel_ms()
    return dev.cpu().numpy()


@pytest.fixture(scope="module")
def tracker(vio, ctx):
    t = vio.Tracker(ctx, TW, TH, max_points=16, max_corners=16)
    yield t
    t.close()


@pytest.mark.parametrize("W,H", [(TW, TH),            # the direct copy
                                 (4 * TW, 4 * TH),    # factor 4 into the slot's pitch
                                 (150, 70)])          # general path
def test_upload_resized_fills_the_slot(vio, ctx, tracker, W, H):
    torch = pytest.importorskip("torch")
    src = strided(W, H, 1, 6)
    rc = vio.lib().erp_tracker_upload_resized(tracker.h, 1, src.ctypes.data_as(C.c_void_p), W, H, src.strides[0])
    assert rc == 0
    got = slot(vio, ctx, torch, tracker, 1)
    np.testing.assert_array_equal(got, ctx.ingest(src, io.GRAY8, 0, TW, TH))
    np.testing.assert_array_equal(got, rgo.resize_area_any(np.ascontiguousarray(src), TW, TH))


@pytest.mark.parametrize("fmt,W,H", [(io.BGR8, 150, 70),     # luma + general resize in one pass
                                     (io.BGRA8, TW, TH),     # convert only at the tracker's size
                                     (io.UYVY, 2 * TW, 2 * TH)])
def test_upload_pixels_fills_the_slot(vio, ctx, tracker, fmt, W, H):
    torch = pytest.importorskip("torch")
    src = strided(W, H, io.BPP[fmt], 7)
    tracker.upload_pixels(0, src, fmt, io.IMREAD)
    got = slot(vio, ctx, torch, tracker, 0)
    np.testing.assert_array_equal(got, ctx.ingest(src, fmt, io.IMREAD, TW, TH))
    np.testing.assert_array_equal(got, io.ingest(src, fmt, io.IMREAD, TW, TH))


@pytest.mark.parametrize("scale", [1, 2])  # a warp of the tracker's size: direct; twice it: warp, then resize
def test_upload_warped_fills_the_slot(vio, ctx, tracker, scale):
    torch = pytest.importorskip("torch")
    sW, sH = 90, 40
    src = strided(sW, sH, 3, 8)
    mx, my = rotated_maps(sW, sH, scale * TW, scale * TH)
    w = ctx.warp_create(mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE)
    try:
        tracker.upload_warped(1, w, src, io.BGR8, io.CVTCOLOR)
        got = slot(vio, ctx, torch, tracker, 1)
        warped = w.apply(src, io.BGR8, io.CVTCOLOR)
        np.testing.assert_array_equal(got, ctx.resize_area_any(warped, TW, TH))
        want = wo.remap(src, io.BGR8, io.CVTCOLOR, mx, my, wo.X_WRAP, wo.Y_REPLICATE)
        np.testing.assert_array_equal(got, rgo.resize_area_any(want, TW, TH))
    finally:
        w.close()


def test_set_mask_from_strided_masks(vio, ctx, tracker):
    m = strided_mask(150, 70, 9)
    tracker.set_mask(m, vio.mask_params(1))
    np.testing.assert_array_equal(tracker.get_mask(), mo.build(m, TW, TH, 1))
    sW, sH = 90, 40
    sm = strided_mask(sW, sH, 10)
    mx, my = rotated_maps(sW, sH, 2 * TW, 2 * TH)
    w = ctx.warp_create(mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE)
    try:
        tracker.set_mask_warped(w, sm, vio.mask_params(1))
        np.testing.assert_array_equal(tracker.get_mask(),
                                      mo.build_warped(sm, mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE, TW, TH, 1))
    finally:
        tracker.set_mask(None)
        w.close()


# ---- kernel timers ----

def test_timers_before_and_after_a_launch(vio):
    L = vio.lib()
    c = vio.Context(0)
    try:
        ms = C.c_double(-1.0)
        for name in ("erp_resize_area_kernel_ms", "erp_equalize_kernel_ms", "erp_mask_kernel_ms",
                     "vio_triangulate_kernel_ms", "vio_mono_init_kernel_ms"):
            assert getattr(L, name)(c.h, C.byref(ms)) == -22, name  # no launch yet
        c.resize_area_any(strided(37, 10, 1, 11), 9, 5)
        c.equalize(strided(35, 18, 1, 12), vio.equalize_params(vio.VIO_EQ_HIST))
        c.mask_build(strided_mask(37, 11, 13), 9, 5, vio.mask_params(1))
        assert c.resize_kernel_ms() > 0 and c.equalize_kernel_ms() > 0 and c.mask_kernel_ms() > 0
    finally:
        c.close()
