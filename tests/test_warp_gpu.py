"""GPU parity of the lens-to-ERP warp (csrc/warp.hip: warp_kernel and its pixel-source variants) against
tests/warp_oracle.py — bitwise: random maps with every border-mode pair, every pixel format and luma rule, strides
and batches, the generators end to end, and the tracker / front-end entry points."""
import ctypes as C

import numpy as np
import pytest

import ingest_oracle as io
import oracle_lib
import resize_general_oracle as rgo
import warp_oracle as wo

pytestmark = pytest.mark.gpu

BORDERS = [(bx, by) for bx in (wo.X_CONSTANT, wo.X_WRAP) for by in (wo.Y_CONSTANT, wo.Y_REPLICATE)]
RULES = (io.CVTCOLOR, io.IMREAD)
FORMATS = (io.GRAY8, io.BGR8, io.RGB8, io.BGRA8, io.RGBA8, io.YUYV, io.UYVY)


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def random_map(sW, sH, dW, dH, seed, pad=3):
    """float32 maps uniform in [-3, S + 3] with the special coordinates injected, as (dH, dW) views of arrays with
    `pad` more columns (map_stride > dW)"""
    rng = np.random.default_rng(seed)
    out = []
    for S in (sW, sH):
        m = np.full((dH, dW + pad), np.float32(-7), np.float32)
        v = rng.uniform(-3, S + 3, dW * dH).astype(np.float32)
        sp = wo.special_coordinates(S)
        pos = rng.choice(v.size, min(sp.size, v.size), replace=False)
        v[pos] = sp[:pos.size]
        m[:, :dW] = v.reshape(dH, dW)
        out.append(m[:, :dW])
    return out


def frame(fmt, W, H, seed=0):
    bgr = np.random.default_rng(1000 + seed + W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return io.from_bgr(bgr, fmt, seed=W)


@pytest.mark.parametrize("bv", [0, 200])
@pytest.mark.parametrize("bx,by", BORDERS)
@pytest.mark.parametrize("sW,sH,dW,dH", [(37, 23, 19, 11),
                                         (64, 48, 300, 7),   # more than one x tile
                                         (5, 4, 1, 1),
                                         (2, 2, 33, 17)])
def test_bitwise_vs_oracle_on_random_maps(ctx, sW, sH, dW, dH, bx, by, bv):
    img = frame(io.GRAY8, sW, sH)
    mx, my = random_map(sW, sH, dW, dH, seed=sW + 7 * dW + bx + by + bv)
    assert mx.strides[0] > 4 * dW
    w = ctx.warp_create(mx, my, sW, sH, bx, by, bv)
    got = w.apply(img)
    w.close()
    np.testing.assert_array_equal(got, wo.remap_grey(img, mx, my, bx, by, bv))


@pytest.mark.parametrize("bx,by", BORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_and_luma_rules(ctx, fmt, bx, by):
    """38 x 23 -> 21 x 9, and a source two pixels wide (the narrowest that takes the pair loads)"""
    for sW, sH in [(38, 23), (2, 3)]:
        dW, dH = 21, 9
        img = frame(fmt, sW, sH)
        mx, my = random_map(sW, sH, dW, dH, seed=fmt + sW)
        w = ctx.warp_create(mx, my, sW, sH, bx, by, 31)
        for rule in RULES:
            np.testing.assert_array_equal(w.apply(img, fmt, rule), wo.remap(img, fmt, rule, mx, my, bx, by, 31))
        w.close()


@pytest.mark.parametrize("bx,by", BORDERS)
def test_one_pixel_wide_source(ctx, bx, by):
    """sW = 1 has no pixel pair: the one-load-per-tap kernels run"""
    for fmt in (io.GRAY8, io.BGR8, io.BGRA8):
        img = frame(fmt, 1, 3)
        mx, my = random_map(1, 3, 70, 5, seed=fmt + bx + by)
        w = ctx.warp_create(mx, my, 1, 3, bx, by, 60)
        np.testing.assert_array_equal(w.apply(img, fmt, io.CVTCOLOR), wo.remap(img, fmt, io.CVTCOLOR, mx, my, bx, by, 60))
        w.close()


def _device_apply(ctx, torch, w, fmt, rule, frames, offset=0, src_pad=0, pitch=None):
    """erp_warp_apply_device on frames `offset` bytes into a torch allocation -> (n, dH, pitch) output"""
    n = len(frames)
    bpp = io.BPP[fmt]
    pitch = w.dW if pitch is None else pitch
    stride = w.sW * bpp + src_pad
    host = np.full((n, w.sH, stride), 255, np.uint8)
    for f in range(n):
        host[f, :, :w.sW * bpp] = frames[f].reshape(w.sH, w.sW * bpp)
    d_buf = torch.zeros(offset + host.size + 16, dtype=torch.uint8, device="cuda:0")
    d_buf[offset:offset + host.size] = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    d_dst = torch.full((n, w.dH, pitch), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    w.apply_device(d_buf.data_ptr() + offset, fmt, rule, stride, n, d_dst.data_ptr(), pitch)
    assert w.kernel_ms() > 0
    return d_dst.cpu().numpy()


@pytest.mark.parametrize("route", ["AUTO", "SINGLE"])
@pytest.mark.parametrize("fmt,offset", [(io.BGRA8, 0), (io.BGRA8, 1), (io.RGBA8, 1), (io.BGR8, 1), (io.YUYV, 1),
                                        (io.GRAY8, 1)])
def test_device_pointer_alignment(vio, ctx, fmt, offset, route):
    """no alignment is asked of src: the pair loads of AUTO at an odd address; under SINGLE aligned BGRA takes the
    dword variant and BGRA at src + 1 the byte variant: the same bytes"""
    torch = pytest.importorskip("torch")
    sW, sH, dW, dH = 38, 23, 21, 9
    img = frame(fmt, sW, sH)
    mx, my = random_map(sW, sH, dW, dH, seed=40 + fmt)
    w = ctx.warp_create(mx, my, sW, sH, wo.X_CONSTANT, wo.Y_REPLICATE, 9)
    w.set_route(getattr(vio, "VIO_WARP_ROUTE_" + route))
    out = _device_apply(ctx, torch, w, fmt, io.IMREAD, [img], offset=offset)
    w.close()
    np.testing.assert_array_equal(out[0], wo.remap(img, fmt, io.IMREAD, mx, my, wo.X_CONSTANT, wo.Y_REPLICATE, 9))


@pytest.mark.parametrize("fmt", [io.GRAY8, io.BGR8, io.BGRA8, io.UYVY])
def test_strides_padding_and_batches(ctx, fmt):
    """stride = sW * bpp + 5 (the bytes past the row end are 255 and must not be read), a padded destination whose
    padding stays intact, and three frames in one launch = three single applies"""
    torch = pytest.importorskip("torch")
    sW, sH, dW, dH = 38, 23, 300, 5
    frames = [frame(fmt, sW, sH, seed=f) for f in range(3)]
    mx, my = random_map(sW, sH, dW, dH, seed=60 + fmt)
    bx, by = wo.X_WRAP, wo.Y_REPLICATE
    w = ctx.warp_create(mx, my, sW, sH, bx, by, 0)
    out = _device_apply(ctx, torch, w, fmt, io.CVTCOLOR, frames, src_pad=5, pitch=dW + 11)
    single = [w.apply(f, fmt, io.CVTCOLOR) for f in frames]
    w.close()
    assert (out[:, :, dW:] == 0xA5).all()
    for f in range(3):
        want = wo.remap(frames[f], fmt, io.CVTCOLOR, mx, my, bx, by, 0)
        if (want == 255).all():
            pytest.fail("the frame would not show a read of the padding")
        np.testing.assert_array_equal(out[f, :, :dW], want)
        np.testing.assert_array_equal(single[f], want)


@pytest.mark.parametrize("bx,by", BORDERS)
@pytest.mark.parametrize("sW,sH", [(38, 23), (2, 3)])
def test_single_route_gives_the_same_bytes(vio, ctx, sW, sH, bx, by):
    """VIO_WARP_ROUTE_SINGLE (one load per tap) against the oracle, every format; 700 columns: three x tiles"""
    dW, dH = 700, 3
    mx, my = random_map(sW, sH, dW, dH, seed=5 + sW + bx + by)
    w = ctx.warp_create(mx, my, sW, sH, bx, by, 140)
    w.set_route(vio.VIO_WARP_ROUTE_SINGLE)
    for fmt in FORMATS:
        img = frame(fmt, sW, sH)
        np.testing.assert_array_equal(w.apply(img, fmt, io.IMREAD), wo.remap(img, fmt, io.IMREAD, mx, my, bx, by, 140))
    w.close()


def test_dual_fisheye_end_to_end(vio, ctx):
    """64 x 32 dual-fisheye -> 48 x 24 ERP; theta_max 80 degrees leaves an uncovered band (invalid pixels)"""
    img = frame(io.BGR8, 64, 32)
    mx, my = vio.warp_map_fisheye(wo.dual_fisheye(80.0), 48, 24, wo.rot_y(0.1234) @ wo.rot_x(0.0567))
    assert np.isnan(mx).any() and not np.isnan(mx).all()
    w = ctx.warp_create(mx, my, 64, 32, wo.X_CONSTANT, wo.Y_CONSTANT, 200)
    got = w.apply(img, io.BGR8, io.IMREAD)
    w.close()
    np.testing.assert_array_equal(got, wo.remap(img, io.BGR8, io.IMREAD, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT, 200))
    assert (got[np.isnan(mx)] == 200).all()


def test_eac_cubemap_end_to_end(vio, ctx):
    img = frame(io.GRAY8, 48, 32)
    mx, my = vio.warp_map_cubemap(wo.cube_faces_3x2(16), 1, 48, 32, 48, 24, wo.rot_y(0.1234) @ wo.rot_x(0.0567))
    w = ctx.warp_create(mx, my, 48, 32)
    got = w.apply(img)
    w.close()
    np.testing.assert_array_equal(got, wo.remap_grey(img, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT))


def test_rejects(vio, ctx):
    """refused on the host, before any launch"""
    mx, my = random_map(40, 24, 10, 6, seed=1)
    w = ctx.warp_create(mx, my, 40, 24)
    with pytest.raises(vio.VioError):
        w.apply(np.zeros((24, 40, 3), np.uint8), io.BGR8, 2)      # unknown luma rule
    with pytest.raises(vio.VioError):
        w.apply(np.zeros((24, 41), np.uint8))                     # not the warp's source size
    assert w.check(7, 0, 400, 10) == -22 and w.check(io.BGR8, 0, 119, 10) == -22 and w.check(io.BGR8, 0, 120, 10) == 0
    w.close()
    with pytest.raises(vio.VioError):
        ctx.warp_create(mx, my, 40, 24, 3, 0)                     # unknown border mode
    w = ctx.warp_create(mx, my, 41, 24)
    with pytest.raises(vio.VioError):
        w.apply(np.zeros((24, 41, 2), np.uint8), io.YUYV)         # odd sW for 4:2:2
    w.close()


# ---- tracker and front end ----

CW, CH, TW, TH = 1440, 720, 960, 480  # camera frames at 1.5x the tracker's size (as tests/test_ingest_gpu.py)
R_CAM = wo.rot_y(0.05) @ wo.rot_x(0.03)  # a tilted mount


def colour_frame(grey):
    g = grey.astype(np.uint16)
    return np.stack([(g * 7) // 8, g, (g * 15) // 16], axis=2).astype(np.uint8)


@pytest.fixture(scope="module")
def rotation_maps(vio):
    """ERP-rotation maps of the camera frame: at the tracker's size (direct) and at the camera's (supersampled)"""
    return {"direct": vio.warp_map_erp(CW, CH, TW, TH, R_CAM), "supersampled": vio.warp_map_erp(CW, CH, CW, CH, R_CAM)}


def oracle_warped(img, maps, route, rule):
    out = wo.remap(img, io.BGR8, rule, maps[route][0], maps[route][1], wo.X_WRAP, wo.Y_REPLICATE)
    return out if route == "direct" else rgo.resize_area_any(out, TW, TH)


@pytest.fixture(scope="module")
def camera_pair(synth):
    A, B, _ = synth.config1(CW, CH)
    return colour_frame(A), colour_frame(B)


@pytest.mark.parametrize("route", ["direct", "supersampled"])
def test_tracker_on_device_warped_frames(vio, gpu_ctx, camera_pair, rotation_maps, route):
    """1440x720 BGR camera frames warped on the device into the tracker's 960x480 slots give bitwise the pipeline
    on the oracle's warped frames"""
    A, B = camera_pair
    a, b = (oracle_warped(x, rotation_maps, route, io.CVTCOLOR) for x in (A, B))
    mask = np.zeros((TH, TW), np.uint8)
    mask[int(np.float32(TH) * np.float32(0.15)):int(np.float32(TH) * (np.float32(1.0) - np.float32(0.15))),
         20:TW - 20] = 255
    pts = oracle_lib.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=78)
    klt = vio.default_klt_params()
    w = gpu_ctx.warp_create(*rotation_maps[route], CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
    res = []
    for warped_on_device in (True, False):
        t = vio.Tracker(gpu_ctx, TW, TH, max_points=1024, max_corners=1024)
        if warped_on_device:
            t.upload_warped(0, w, A, vio.VIO_PIX_BGR8, vio.VIO_LUMA_CVTCOLOR)
            t.upload_warped(1, w, B, vio.VIO_PIX_BGR8, vio.VIO_LUMA_CVTCOLOR)
        else:
            t.upload(0, a)
            t.upload(1, b)
        t.set_points(pts)
        t.run(prm, klt)
        res.append(t.download())
        t.close()
    w.close()
    for k in ("status", "next", "kept", "corners"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert res[0]["kept"].sum() > 100  # the pair really is tracked


@pytest.mark.parametrize("route", ["direct", "supersampled"])
def test_upload_warped_fills_the_slot(vio, gpu_ctx, camera_pair, rotation_maps, route):
    """the slot holds the oracle's warped (and resized) frame"""
    torch = pytest.importorskip("torch")
    A = camera_pair[0]
    w = gpu_ctx.warp_create(*rotation_maps[route], CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
    t = vio.Tracker(gpu_ctx, TW, TH, max_points=16, max_corners=16)
    t.upload_warped(1, w, A, vio.VIO_PIX_BGR8, vio.VIO_LUMA_IMREAD)
    ptr, pitch = C.c_void_p(), C.c_int()
    gpu_ctx.check(vio.lib().erp_tracker_device_frame(t.h, 1, C.byref(ptr), C.byref(pitch)), "erp_tracker_device_frame")
    dev = torch.zeros((TH, TW), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.resize_area_any_device(ptr.value, TW, TH, pitch.value, 1, dev.data_ptr(), TW, TH, TW)  # a 1:1 copy
    gpu_ctx.resize_kernel_ms()
    np.testing.assert_array_equal(dev.cpu().numpy(), oracle_warped(A, rotation_maps, route, io.IMREAD))
    t.close()
    w.close()


@pytest.fixture(scope="module")
def camera_sequence(synth):
    return [colour_frame(synth.render_erp(CW, CH, synth.rot_yaw_pitch(1.2 * f, 0.3 * f))) for f in range(3)]


@pytest.mark.parametrize("route", ["direct", "supersampled"])
def test_frontend_track_warped(vio, gpu_ctx, camera_sequence, rotation_maps, route):
    """three 1440x720 BGR frames through Frontend.track_warped = Frontend.track on the oracle's warped frames"""
    prm = vio.default_frontend_params(seed=11)
    fe_cam = vio.Frontend(gpu_ctx, TW, TH, prm)
    fe_ref = vio.Frontend(gpu_ctx, TW, TH, prm)
    w = gpu_ctx.warp_create(*rotation_maps[route], CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
    carried = 0
    for f, img in enumerate(camera_sequence):
        g = fe_cam.track_warped(w, img, vio.VIO_PIX_BGR8, vio.VIO_LUMA_IMREAD)
        o = fe_ref.track(oracle_warped(img, rotation_maps, route, io.IMREAD))
        assert np.array_equal(g["ids"], o["ids"]), f
        assert np.array_equal(g["xy"], o["xy"]), f
        assert np.array_equal(g["track_count"], o["track_count"]), f
        assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f
        if f:
            carried += int((g["track_count"] > 0).sum())
    fe_cam.close()
    fe_ref.close()
    w.close()
    assert carried > 100  # features really are carried across frames


def test_upload_warped_rejects(vio, gpu_ctx):
    L = vio.lib()
    img = np.zeros((CH, CW), np.uint8)
    p = img.ctypes.data_as(C.c_void_p)
    t = vio.Tracker(gpu_ctx, TW, TH, max_points=16, max_corners=16)
    fe = vio.Frontend(gpu_ctx, TW, TH)
    other = vio.Context(0)
    try:
        w = other.warp_create(*vio.warp_map_erp(CW, CH, TW, TH), CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
        assert L.erp_tracker_upload_warped(t.h, 0, w.h, p, io.GRAY8, 0, CW) == -22   # another context
        assert L.erp_frontend_track_warped(fe.h, w.h, p, io.GRAY8, 0, CW, None) == -22
        w.close()
    finally:
        other.close()
    for dW, dH in [(TW - 1, TH), (TW, TH - 1), (TW // 2, TH // 2), (2 * TW, TH - 1)]:
        w = gpu_ctx.warp_create(*vio.warp_map_erp(CW, CH, dW, dH), CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
        assert L.erp_tracker_upload_warped(t.h, 0, w.h, p, io.GRAY8, 0, CW) == -38   # smaller than the tracker
        assert L.erp_frontend_track_warped(fe.h, w.h, p, io.GRAY8, 0, CW, None) == -38
        w.close()
    w = gpu_ctx.warp_create(*vio.warp_map_erp(CW, CH, TW, TH), CW, CH, wo.X_WRAP, wo.Y_REPLICATE)
    assert L.erp_tracker_upload_warped(t.h, 2, w.h, p, io.GRAY8, 0, CW) == -22       # no such slot
    assert L.erp_tracker_upload_warped(t.h, 0, w.h, p, io.GRAY8, 0, CW - 1) == -22   # stride < sW
    assert L.erp_tracker_upload_warped(t.h, 0, w.h, p, io.GRAY8, 0, CW) == 0
    t.sync()
    w.close()
    fe.close()
    t.close()
