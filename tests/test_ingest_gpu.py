"""GPU parity of the colour / packed-YUV ingest (csrc/resize.hip: ingest_convert_kernel and the pixel-source
variants of the area kernels) against tests/ingest_oracle.py — bitwise.  erp_ingest = erp_resize_area_any of the
grey image that the luma rule makes of the packed frame, for every format, path, load variant and route."""
import numpy as np
import pytest

import ingest_oracle as io
import oracle_lib
import resize_general_oracle as rgo

pytestmark = pytest.mark.gpu

RULES = (io.CVTCOLOR, io.IMREAD)
CONVERT = [(37, 23, 37, 23)]
INTEGER = [(40, 24, 10, 6),    # factor 4, aligned
           (44, 20, 11, 5),    # factor 4, dW % 4 != 0
           (30, 14, 15, 7),    # the 2x2 rule
           (35, 21, 7, 7)]     # factors 5 x 3
GENERAL = [(37, 23, 11, 7),
           (64, 48, 64, 20),     # x identity
           (1001, 3, 1000, 2),   # the sliver rule
           (1100, 70, 257, 17),  # more than one x tile
           (50, 23, 21, 9), (39, 23, 10, 9), (69, 23, 10, 9), (79, 23, 10, 9), (200, 23, 21, 9)]  # 4, 5, 8, 9, 11 taps
SHAPES = CONVERT + INTEGER + GENERAL


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def rand_bgr(W, H, seed=None):
    return np.random.default_rng(W + H if seed is None else seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def frame(fmt, W, H, seed=None):
    return io.from_bgr(rand_bgr(W, H, seed), fmt, seed=W)


@pytest.mark.parametrize("fmt", [io.BGR8, io.BGRA8])
@pytest.mark.parametrize("W,H,dW,dH", SHAPES)
def test_bitwise_vs_oracle(ctx, fmt, W, H, dW, dH):
    img = frame(fmt, W, H)
    rule = (W + fmt) % 2  # both rules on every path, for both formats
    np.testing.assert_array_equal(ctx.ingest(img, fmt, rule, dW, dH), io.ingest(img, fmt, rule, dW, dH))


@pytest.mark.parametrize("fmt", [io.RGB8, io.RGBA8, io.YUYV, io.UYVY, io.GRAY8])
@pytest.mark.parametrize("W,H,dW,dH", [(38, 23, 38, 23), (40, 24, 10, 6), (30, 14, 15, 7), (38, 23, 11, 7),
                                       (70, 23, 10, 9)])
def test_other_formats(ctx, fmt, W, H, dW, dH):
    """convert only, factor 4, 2 x 2, and the general path's <4> and <8> variants; even widths for 4:2:2"""
    img = frame(fmt, W, H)
    for rule in RULES:
        np.testing.assert_array_equal(ctx.ingest(img, fmt, rule, dW, dH), io.ingest(img, fmt, rule, dW, dH))


def test_gray8_is_resize_area_any(ctx):
    img = np.random.default_rng(2).integers(0, 256, (23, 37), dtype=np.uint8)
    for dW, dH in [(37, 23), (11, 7)]:
        np.testing.assert_array_equal(ctx.ingest(img, io.GRAY8, 0, dW, dH), ctx.resize_area_any(img, dW, dH))


@pytest.fixture(scope="module")
def all_triples():
    """4096 x 4096 BGR8 holding every triple once"""
    v = np.arange(256, dtype=np.uint8)
    img = np.empty((256, 256, 256, 3), np.uint8)
    img[..., 0] = v[:, None, None]
    img[..., 1] = v[None, :, None]
    img[..., 2] = v[None, None, :]
    return img.reshape(4096, 4096, 3)


@pytest.mark.parametrize("rule", RULES)
def test_convert_all_bgr_triples(ctx, all_triples, rule):
    np.testing.assert_array_equal(ctx.ingest(all_triples, io.BGR8, rule, 4096, 4096),
                                  io.luma(all_triples, io.BGR8, rule))


@pytest.mark.parametrize("route", ["FUSED", "TWO_PASS", "FUSED_BYTES"])
@pytest.mark.parametrize("fmt", [io.BGR8, io.BGRA8, io.UYVY])
def test_every_route_gives_the_same_bytes(vio, ctx, route, fmt):
    ctx.set_ingest_route(getattr(vio, "VIO_INGEST_ROUTE_" + route))
    try:
        for W, H, dW, dH in [(40, 24, 10, 6), (30, 14, 15, 7), (30, 21, 6, 7), (38, 23, 11, 7), (70, 23, 10, 9),
                             (200, 23, 21, 9), (38, 23, 38, 23)]:  # even widths: UYVY
            img = frame(fmt, W, H)
            np.testing.assert_array_equal(ctx.ingest(img, fmt, 1, dW, dH), io.ingest(img, fmt, 1, dW, dH))
    finally:
        ctx.set_ingest_route(vio.VIO_INGEST_ROUTE_AUTO)


@pytest.mark.parametrize("fmt", [io.BGR8, io.BGRA8, io.YUYV])
@pytest.mark.parametrize("W,H,dW,dH", [(40, 24, 10, 6), (38, 23, 11, 7), (38, 23, 38, 23)])
def test_strided_source(ctx, fmt, W, H, dW, dH):
    """row stride W * bpp + 5; the bytes past the row end are 255 and must not be read"""
    bpp = io.BPP[fmt]
    img = frame(fmt, W, H)
    buf = np.full((H, W * bpp + 5), 255, np.uint8)
    buf[:, :W * bpp] = img.reshape(H, W * bpp)
    view = np.lib.stride_tricks.as_strided(buf, shape=(H, W, bpp), strides=(W * bpp + 5, bpp, 1))
    want = io.ingest(img, fmt, 0, dW, dH)
    if (want == 255).all():
        pytest.fail("the frame would not show a read of the padding")
    np.testing.assert_array_equal(ctx.ingest(view, fmt, 0, dW, dH), want)


def _device_case(ctx, torch, fmt, W, H, dW, dH, offset, n_frames=1, pitch=None, src_pad=0):
    """erp_ingest_device on frames at `offset` bytes into a torch allocation -> (frames, (n, dH, pitch) output)"""
    bpp = io.BPP[fmt]
    pitch = dW if pitch is None else pitch
    stride = W * bpp + src_pad
    frames = [frame(fmt, W, H, seed=11 + f) for f in range(n_frames)]
    host = np.full((n_frames, H, stride), 255, np.uint8)
    for f in range(n_frames):
        host[f, :, :W * bpp] = frames[f].reshape(H, W * bpp)
    d_buf = torch.zeros(offset + host.size + 16, dtype=torch.uint8, device="cuda:0")
    d_buf[offset:offset + host.size] = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    d_dst = torch.full((n_frames, dH, pitch), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.ingest_device(d_buf.data_ptr() + offset, fmt, 0, W, H, stride, n_frames, d_dst.data_ptr(), dW, dH, pitch)
    assert ctx.resize_kernel_ms() > 0
    return frames, d_dst.cpu().numpy()


@pytest.mark.parametrize("fmt", [io.BGRA8, io.BGR8])
@pytest.mark.parametrize("W,H,dW,dH", [(40, 24, 10, 6), (38, 23, 11, 7), (37, 23, 37, 23)])
def test_device_pointer_offset_by_one_byte(ctx, fmt, W, H, dW, dH):
    """a source 1 byte off a torch allocation: BGRA takes the byte variant (the dword variant needs src % 4 == 0)"""
    torch = pytest.importorskip("torch")
    frames, out = _device_case(ctx, torch, fmt, W, H, dW, dH, offset=1)
    np.testing.assert_array_equal(out[0], io.ingest(frames[0], fmt, 0, dW, dH))


@pytest.mark.parametrize("W,H,dW,dH", [(40, 24, 10, 6), (38, 23, 11, 7), (37, 23, 37, 23)])
def test_aligned_bgra_takes_the_dword_variant(ctx, W, H, dW, dH):
    """src and stride multiples of 4"""
    torch = pytest.importorskip("torch")
    frames, out = _device_case(ctx, torch, io.BGRA8, W, H, dW, dH, offset=0)
    np.testing.assert_array_equal(out[0], io.ingest(frames[0], io.BGRA8, 0, dW, dH))


@pytest.mark.parametrize("fmt", [io.BGR8, io.BGRA8])
@pytest.mark.parametrize("W,H,dW,dH", [(40, 24, 10, 6), (100, 37, 30, 11), (37, 23, 37, 23)])
def test_device_batched_frames_with_padded_destination(ctx, fmt, W, H, dW, dH):
    torch = pytest.importorskip("torch")
    frames, out = _device_case(ctx, torch, fmt, W, H, dW, dH, offset=0, n_frames=3, pitch=dW + 10, src_pad=5)
    for f in range(3):
        np.testing.assert_array_equal(out[f, :, :dW], io.ingest(frames[f], fmt, 0, dW, dH))
    assert (out[:, :, dW:] == 0xA5).all()  # the padding of the destination rows is untouched


@pytest.mark.parametrize("fmt", [io.BGR8, io.BGRA8, io.YUYV])
def test_saturated_frames(ctx, fmt):
    for v in (255, 0):
        for dW, dH in [(30, 11), (25, 37), (100, 37)]:
            out = ctx.ingest(np.full((37, 100, io.BPP[fmt]), v, np.uint8), fmt, 0, dW, dH)
            assert (out == v).all(), (v, dW, dH, np.unique(out))


def test_table_cache_follows_the_sizes(ctx):
    """two size pairs and two formats in turn on one context: each call uses its own tap tables"""
    a, b = frame(io.BGR8, 100, 37), frame(io.BGRA8, 90, 60)
    for _ in range(2):
        np.testing.assert_array_equal(ctx.ingest(a, io.BGR8, 0, 30, 11), io.ingest(a, io.BGR8, 0, 30, 11))
        np.testing.assert_array_equal(ctx.ingest(b, io.BGRA8, 0, 30, 17), io.ingest(b, io.BGRA8, 0, 30, 17))


def test_rejects(vio, ctx):
    """refused on the host, before any launch"""
    img = np.zeros((24, 40, 3), np.uint8)
    with pytest.raises(vio.VioError):
        ctx.ingest(img, io.BGR8, 0, 41, 24)  # enlarging
    with pytest.raises(vio.VioError):
        ctx.ingest(img, io.BGR8, 0, 40, 25)
    with pytest.raises(vio.VioError):
        ctx.ingest(img, 7, 0, 10, 6)  # unknown format
    with pytest.raises(vio.VioError):
        ctx.ingest(img, io.BGR8, 2, 10, 6)  # unknown luma rule
    with pytest.raises(vio.VioError):
        ctx.ingest(np.zeros((24, 41, 2), np.uint8), io.YUYV, 0, 10, 6)  # odd W for 4:2:2
    rc = vio.lib().erp_ingest(ctx.h, img.ctypes.data_as(vio.C.c_void_p), io.BGR8, 0, 40, 24, 119,
                              img.ctypes.data_as(vio.C.c_void_p), 10, 6, 10)  # stride < W * bpp
    assert rc == -22 and b"bad sizes" in vio.lib().vio_ctx_last_error(ctx.h)


CW, CH, TW, TH = 1440, 720, 960, 480  # camera frames at 1.5x the tracker's size


def colour_frame(grey):
    """a BGR frame from a grey one: three differently scaled copies, no channel uniform"""
    g = grey.astype(np.uint16)
    return np.stack([(g * 7) // 8, g, (g * 15) // 16], axis=2).astype(np.uint8)


@pytest.fixture(scope="module")
def camera_pair(synth):
    A, B, _ = synth.config1(CW, CH)
    A, B = colour_frame(A), colour_frame(B)
    return A, B, io.ingest(A, io.BGR8, io.CVTCOLOR, TW, TH), io.ingest(B, io.BGR8, io.CVTCOLOR, TW, TH)


def test_tracker_on_device_ingested_frames(vio, gpu_ctx, camera_pair):
    """1440x720 BGR camera frames ingested on the device into the tracker's 960x480 slots give bitwise the
    pipeline on the oracle's grey frames."""
    A, B, a, b = camera_pair
    for c in range(3):
        assert A[..., c].min() != A[..., c].max()
    mask = np.zeros((TH, TW), np.uint8)
    mask[int(np.float32(TH) * np.float32(0.15)):int(np.float32(TH) * (np.float32(1.0) - np.float32(0.15))),
         20:TW - 20] = 255
    pts = oracle_lib.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=78)
    klt = vio.default_klt_params()
    res = []
    for ingested_on_device in (True, False):
        t = vio.Tracker(gpu_ctx, TW, TH, max_points=1024, max_corners=1024)
        if ingested_on_device:
            t.upload_pixels(0, A, vio.VIO_PIX_BGR8, vio.VIO_LUMA_CVTCOLOR)
            t.upload_pixels(1, B, vio.VIO_PIX_BGR8, vio.VIO_LUMA_CVTCOLOR)
        else:
            t.upload(0, a)
            t.upload(1, b)
        t.set_points(pts)
        t.run(prm, klt)
        res.append(t.download())
        t.close()
    for k in ("status", "next", "kept", "corners"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert res[0]["kept"].sum() > 200


def test_tracker_upload_pixels_at_tracker_size(vio, gpu_ctx):
    """a frame already at the tracker's size takes the convert-only pass: the slot holds the oracle's luma"""
    torch = pytest.importorskip("torch")
    img = frame(io.RGBA8, TW, TH)
    t = vio.Tracker(gpu_ctx, TW, TH, max_points=16, max_corners=16)
    t.upload_pixels(0, img, vio.VIO_PIX_RGBA8, vio.VIO_LUMA_IMREAD)
    ptr, pitch = vio.C.c_void_p(), vio.C.c_int()
    gpu_ctx.check(vio.lib().erp_tracker_device_frame(t.h, 0, vio.C.byref(ptr), vio.C.byref(pitch)),
                  "erp_tracker_device_frame")
    dev = torch.zeros((TH, TW), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.resize_area_any_device(ptr.value, TW, TH, pitch.value, 1, dev.data_ptr(), TW, TH, TW)  # a 1:1 copy
    gpu_ctx.resize_kernel_ms()
    np.testing.assert_array_equal(dev.cpu().numpy(), io.luma(img, io.RGBA8, io.IMREAD))
    t.close()


def test_frontend_track_pixels(vio, synth, gpu_ctx):
    """three 1440x720 BGR frames through Frontend.track_pixels = Frontend.track on the oracle's grey frames"""
    prm = vio.default_frontend_params(seed=11)
    fe_cam = vio.Frontend(gpu_ctx, TW, TH, prm)
    fe_ref = vio.Frontend(gpu_ctx, TW, TH, prm)
    carried = 0
    for f in range(3):
        img = colour_frame(synth.render_erp(CW, CH, synth.rot_yaw_pitch(1.2 * f, 0.3 * f)))
        g = fe_cam.track_pixels(img, vio.VIO_PIX_BGR8, vio.VIO_LUMA_IMREAD)
        o = fe_ref.track(io.ingest(img, io.BGR8, io.IMREAD, TW, TH))
        assert np.array_equal(g["ids"], o["ids"]), f
        assert np.array_equal(g["xy"], o["xy"]), f
        assert np.array_equal(g["track_count"], o["track_count"]), f
        assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f
        if f:
            carried += int((g["track_count"] > 0).sum())
    fe_cam.close()
    fe_ref.close()
    assert carried > 100  # features really are carried across frames
