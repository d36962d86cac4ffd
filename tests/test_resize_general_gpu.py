"""GPU parity of erp_resize_area_any (csrc/resize.hip, resize_area_general_kernel) against
tests/resize_general_oracle.py — bitwise.  cv::resize(..., INTER_AREA) of the frames (app/main.cpp:203) for
sizes that are no integer fraction of the camera's."""
import numpy as np
import pytest

import oracle_lib
import resize_general_oracle as rgo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def rand_img(W, H, seed=None):
    return np.random.default_rng(W + H if seed is None else seed).integers(0, 256, (H, W), dtype=np.uint8)


@pytest.mark.parametrize("W,H,dW,dH", [
    (7, 5, 3, 2),
    (100, 37, 30, 11),
    (64, 48, 64, 20),      # x identity, y fractional
    (90, 60, 30, 17),      # x integer 3, y fractional
    (33, 17, 32, 16),
    (1001, 3, 1000, 2),    # the sliver rule
    (1100, 70, 257, 17),   # more than one x tile, ragged tail
    (960, 480, 640, 320),
])
def test_bitwise_vs_oracle(ctx, W, H, dW, dH):
    img = rand_img(W, H)
    np.testing.assert_array_equal(ctx.resize_area_any(img, dW, dH), rgo.resize_area_any(img, dW, dH))


@pytest.mark.parametrize("W,dW,taps", [(50, 21, 4), (39, 10, 5), (69, 10, 8), (79, 10, 9), (200, 21, 11)])
def test_every_tap_count_variant(ctx, W, dW, taps):
    """the kernel has a variant for columns of at most 4 taps, one for at most 8 and one for any count: sizes
    whose widest column has exactly 4, 5, 8, 9 and 11 taps"""
    assert np.bincount(rgo.area_tab(W, dW)[0]).max() == taps
    img = rand_img(W, 23)
    np.testing.assert_array_equal(ctx.resize_area_any(img, dW, 9), rgo.resize_area_any(img, dW, 9))


@pytest.mark.parametrize("W,H,dW,dH", [(100, 40, 20, 8), (960, 480, 480, 240), (64, 48, 64, 48)])
def test_integer_factors_equal_resize_area(ctx, W, H, dW, dH):
    img = rand_img(W, H)
    np.testing.assert_array_equal(ctx.resize_area_any(img, dW, dH), ctx.resize_area(img, dW, dH))


def test_strided_source(ctx):
    big = np.zeros((480, 1000), np.uint8)
    big[:, :960] = rand_img(960, 480, seed=1)
    big[:, 960:] = 255  # bytes past the row end must not be read
    view = big[:, :960]  # row stride 1000
    np.testing.assert_array_equal(ctx.resize_area_any(view, 640, 320),
                                  rgo.resize_area_any(np.ascontiguousarray(view), 640, 320))


def test_device_batched_frames_with_padded_destination(ctx):
    torch = pytest.importorskip("torch")
    W, H, dW, dH, pitch = 100, 37, 30, 11, 40
    frames = np.random.default_rng(7).integers(0, 256, (3, H, W), dtype=np.uint8)
    d_src = torch.from_numpy(frames).to("cuda:0")
    d_dst = torch.full((3, dH, pitch), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.resize_area_any_device(d_src.data_ptr(), W, H, W, 3, d_dst.data_ptr(), dW, dH, pitch)
    assert ctx.resize_kernel_ms() > 0
    out = d_dst.cpu().numpy()
    for f in range(3):
        np.testing.assert_array_equal(out[f, :, :dW], rgo.resize_area_any(frames[f], dW, dH))
    assert (out[:, :, dW:] == 0xA5).all()  # the padding of the destination rows is untouched


def test_saturated_frames(ctx):
    for v in (255, 0):
        out = ctx.resize_area_any(np.full((37, 100), v, np.uint8), 30, 11)
        assert (out == v).all(), (v, np.unique(out))


def test_table_cache_follows_the_sizes(ctx):
    """two size pairs in turn on one context: each call uses its own tap tables"""
    a, b = rand_img(100, 37), rand_img(90, 60)
    for _ in range(2):
        np.testing.assert_array_equal(ctx.resize_area_any(a, 30, 11), rgo.resize_area_any(a, 30, 11))
        np.testing.assert_array_equal(ctx.resize_area_any(b, 30, 17), rgo.resize_area_any(b, 30, 17))


def test_enlarging_rejected(vio, ctx):
    with pytest.raises(vio.VioError):
        ctx.resize_area_any(np.zeros((480, 960), np.uint8), 1000, 480)
    with pytest.raises(vio.VioError):
        ctx.resize_area_any(np.zeros((480, 960), np.uint8), 960, 481)


CW, CH, TW, TH = 1440, 720, 960, 480  # camera frames at 1.5x the tracker's size


@pytest.fixture(scope="module")
def camera_pair(synth):
    A, B, _ = synth.config1(CW, CH)
    return A, B, rgo.resize_area_any(A, TW, TH), rgo.resize_area_any(B, TW, TH)


def test_tracker_on_device_resized_frames(vio, gpu_ctx, camera_pair):
    """1440x720 camera frames resized on the device into the tracker's 960x480 slots give bitwise the
    pipeline on oracle-resized frames."""
    A, B, a, b = camera_pair
    mask = np.zeros((TH, TW), np.uint8)
    mask[int(np.float32(TH) * np.float32(0.15)):int(np.float32(TH) * (np.float32(1.0) - np.float32(0.15))),
         20:TW - 20] = 255
    pts = oracle_lib.gftt(a, mask, 300, float(np.float32(0.01)), 30.0)
    prm = vio.default_tracker_params(max_corners=300, seed=78)
    klt = vio.default_klt_params()
    res = []
    for resized_on_device in (True, False):
        t = vio.Tracker(gpu_ctx, TW, TH, max_points=1024, max_corners=1024)
        if resized_on_device:
            t.upload_resized(0, A)
            t.upload_resized(1, B)
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


def test_frontend_track_resized(vio, synth, gpu_ctx):
    """three 1440x720 frames through Frontend.track_resized = Frontend.track on the oracle-resized frames"""
    prm = vio.default_frontend_params(seed=11)
    fe_cam = vio.Frontend(gpu_ctx, TW, TH, prm)
    fe_ref = vio.Frontend(gpu_ctx, TW, TH, prm)
    carried = 0
    for f in range(3):
        img = synth.render_erp(CW, CH, synth.rot_yaw_pitch(1.2 * f, 0.3 * f))
        g = fe_cam.track_resized(img)
        o = fe_ref.track(rgo.resize_area_any(img, TW, TH))
        assert np.array_equal(g["ids"], o["ids"]), f
        assert np.array_equal(g["xy"], o["xy"]), f
        assert np.array_equal(g["track_count"], o["track_count"]), f
        assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f
        if f:
            carried += int((g["track_count"] > 0).sum())
    fe_cam.close()
    fe_ref.close()
    assert carried > 100  # features really are carried across frames
