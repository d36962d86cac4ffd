"""GPU parity of the contrast equalisation (csrc/equalize.hip: eq_hist_kernel, eq_lut_kernel, eq_apply_kernel) against
tests/equalize_oracle.py — bitwise: CLAHE over divisible and extended tilings, clip limits and image kinds, HIST, the
horizontal wrap, strides / alignment / batches / in place, and the tracker and front-end entry points."""
import ctypes as C

import numpy as np
import pytest

import equalize_oracle as eo

pytestmark = pytest.mark.gpu

TW, TH = 960, 480  # the front-end GPU tests' size
SIZES = [(64, 32, 8, 8),    # 8 x 4 tiles of 32 pixels: c = 1 at every clip limit of the sweep but 40
         (37, 23, 4, 3),    # both axes extended
         (40, 23, 4, 3),    # width divisible, height not: the width still grows by a whole tiles count
         (96, 48, 8, 8),
         (1100, 70, 8, 8),  # 138 x 9 tiles: several apply rectangles in x
         (1100, 70, 2, 2),  # 550 x 35 tiles: a tile's histogram is split over 9 workgroups (HIST: the frame's over 35,
                            # more than the 16 lane groups that sum them)
         (2, 2, 1, 1)]
CLIPS = (0, 0.01, 3, 40)
KINDS = ("noise", "constant", "narrow", "ramp")


@pytest.fixture(scope="module")
def ctx(vio):
    c = vio.Context(0)
    yield c
    c.close()


def image(kind, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 93, np.uint8)
    if kind == "narrow":
        return rng.integers(100, 111, (H, W), dtype=np.uint8)
    assert kind == "ramp"
    return np.broadcast_to((np.arange(W) * 255 // (W - 1)).astype(np.uint8), (H, W)).copy()


def clahe_params(vio, tx=8, ty=8, clip=3.0, border_x=eo.X_CLAMP):
    return vio.equalize_params(vio.VIO_EQ_CLAHE, tx, ty, clip, border_x)


@pytest.mark.parametrize("W,H,tx,ty", SIZES)
def test_clahe_bitwise_vs_oracle(vio, ctx, W, H, tx, ty):
    for kind in KINDS:
        img = image(kind, W, H)
        for clip in CLIPS:
            got = ctx.equalize(img, clahe_params(vio, tx, ty, clip))
            np.testing.assert_array_equal(got, eo.clahe(img, tx, ty, clip), err_msg=f"{kind} clip {clip}")
    assert ctx.equalize_kernel_ms() > 0


def test_small_tiles_sit_at_the_clip_floor():
    """the 64 x 32 case's 32-pixel tiles: c = max(int(clip * 32 / 256), 1) = 1 for clip 0.01 and 3"""
    assert [eo.clahe_clip(np.zeros(256, int), 32, c)[1]["c"] for c in CLIPS] == [0, 1, 1, 5]


@pytest.mark.parametrize("W,H,tx,ty", SIZES)
def test_hist_bitwise_vs_oracle(vio, ctx, W, H, tx, ty):
    p = vio.equalize_params(vio.VIO_EQ_HIST)
    for kind in KINDS:
        img = image(kind, W, H)
        np.testing.assert_array_equal(ctx.equalize(img, p), eo.equalize_hist(img), err_msg=kind)
    const = image("constant", W, H)
    np.testing.assert_array_equal(ctx.equalize(const, p), const)  # a single-bin frame keeps its value


@pytest.mark.parametrize("W,H", [(64, 32), (96, 48)])
def test_wrap_bitwise_vs_oracle(vio, ctx, W, H):
    for kind in KINDS:
        img = image(kind, W, H)
        for clip in CLIPS:
            got = ctx.equalize(img, clahe_params(vio, 8, 8, clip, eo.X_WRAP))
            np.testing.assert_array_equal(got, eo.clahe(img, 8, 8, clip, eo.X_WRAP), err_msg=f"{kind} clip {clip}")
    img = image("noise", W, H)
    wrap = ctx.equalize(img, clahe_params(vio, 8, 8, 3.0, eo.X_WRAP))
    clamp = ctx.equalize(img, clahe_params(vio, 8, 8, 3.0, eo.X_CLAMP))
    assert np.any(wrap[:, 0] != clamp[:, 0]) and np.any(wrap[:, W - 1] != clamp[:, W - 1])  # the seam really differs


def test_none_is_a_copy(vio, ctx):
    img = image("noise", 37, 23)
    np.testing.assert_array_equal(ctx.equalize(img, vio.equalize_params(vio.VIO_EQ_NONE)), img)


def test_host_stride(vio, ctx):
    """Context.equalize honours the rows' stride of a view"""
    W, H = 37, 23
    big = np.full((H, W + 5), 255, np.uint8)
    big[:, :W] = image("noise", W, H)
    view = big[:, :W]
    assert view.strides[0] == W + 5
    np.testing.assert_array_equal(ctx.equalize(view, clahe_params(vio, 4, 3)), eo.clahe(view, 4, 3, 3.0))


def _device_run(ctx, torch, frames, p, src_pad=0, dst_pad=0, src_off=0, dst_off=0, in_place=False):
    """erp_equalize_device on frames with rows of W + src_pad bytes, src_off bytes into a torch allocation ->
    (n, H, W + dst_pad) destination bytes (0xA5 where nothing was written)"""
    n = len(frames)
    H, W = frames[0].shape
    stride = W + src_pad
    host = np.full((n, H, stride), 0x5A, np.uint8)
    for f in range(n):
        host[f, :, :W] = frames[f]
    d_src = torch.zeros(src_off + host.size + 16, dtype=torch.uint8, device="cuda:0")
    d_src[src_off:src_off + host.size] = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    if in_place:
        torch.cuda.synchronize()
        ctx.equalize_device(d_src.data_ptr() + src_off, W, H, stride, n, p, d_src.data_ptr() + src_off, stride)
        assert ctx.equalize_kernel_ms() > 0
        return d_src[src_off:src_off + host.size].cpu().numpy().reshape(n, H, stride)
    pitch = W + dst_pad
    d_dst = torch.full((dst_off + n * H * pitch + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.equalize_device(d_src.data_ptr() + src_off, W, H, stride, n, p, d_dst.data_ptr() + dst_off, pitch)
    assert ctx.equalize_kernel_ms() > 0
    out = d_dst.cpu().numpy()
    assert np.all(out[:dst_off] == 0xA5) and np.all(out[dst_off + n * H * pitch:] == 0xA5)
    return out[dst_off:dst_off + n * H * pitch].reshape(n, H, pitch)


@pytest.mark.parametrize("mode", ["clahe", "hist"])
@pytest.mark.parametrize("W,H,tx,ty", [(37, 23, 4, 3), (1100, 70, 8, 8)])
def test_device_layouts(vio, ctx, W, H, tx, ty, mode):
    """source stride W + 5, a padded destination whose padding keeps its sentinel, odd base addresses, a 3-frame
    batch equal to three single calls, in place equal to out of place"""
    torch = pytest.importorskip("torch")
    p = clahe_params(vio, tx, ty) if mode == "clahe" else vio.equalize_params(vio.VIO_EQ_HIST)
    frames = [image("noise", W, H), image("narrow", W, H), image("ramp", W, H)]
    want = [eo.clahe(f, tx, ty, 3.0) if mode == "clahe" else eo.equalize_hist(f) for f in frames]
    # stride, destination padding and odd addresses, one frame
    out = _device_run(ctx, torch, frames[:1], p, src_pad=5, dst_pad=7, src_off=1, dst_off=3)
    np.testing.assert_array_equal(out[0, :, :W], want[0])
    assert np.all(out[0, :, W:] == 0xA5)
    # the batch = three single calls (and the oracle), each frame equalised on its own
    batch = _device_run(ctx, torch, frames, p, src_pad=5, dst_pad=2, src_off=1)
    for f in range(3):
        single = _device_run(ctx, torch, frames[f:f + 1], p, src_pad=5, dst_pad=2, src_off=1)
        np.testing.assert_array_equal(batch[f], single[0])
        np.testing.assert_array_equal(batch[f, :, :W], want[f])
    assert np.all(batch[:, :, W:] == 0xA5)
    # in place: the same bytes, the source's padding untouched
    inp = _device_run(ctx, torch, frames, p, src_pad=5, src_off=3, in_place=True)
    for f in range(3):
        np.testing.assert_array_equal(inp[f, :, :W], want[f])
    assert np.all(inp[:, :, W:] == 0x5A)


def test_device_rejects(vio, ctx):
    torch = pytest.importorskip("torch")
    L = vio.lib()
    buf = torch.zeros(64 * 32 * 2, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s = buf.data_ptr()
    good = clahe_params(vio)
    for p, W, H, st, dst, dst_st in [(clahe_params(vio, 8, 8, 3.0, eo.X_WRAP), 60, 32, 64, s + 2048, 64),  # not divisible
                                     (clahe_params(vio, 33, 8), 64, 32, 64, s + 2048, 64),
                                     (clahe_params(vio, 8, 8, -1.0), 64, 32, 64, s + 2048, 64),
                                     (good, 64, 32, 63, s + 2048, 64),
                                     (good, 60, 32, 64, s, 62)]:  # in place with another stride
        assert L.erp_equalize_device(ctx.h, s, W, H, st, 1, C.byref(p), dst, dst_st) == -22
    assert L.erp_equalize_device(ctx.h, s, 64, 32, 64, 0, C.byref(good), s + 2048, 64) == 0  # no frames: nothing to do


def _slot(vio, ctx, torch, t, slot):
    ptr, pitch = C.c_void_p(), C.c_int()
    ctx.check(vio.lib().erp_tracker_device_frame(t.h, slot, C.byref(ptr), C.byref(pitch)), "erp_tracker_device_frame")
    dev = torch.zeros((t.H, t.W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.resize_area_any_device(ptr.value, t.W, t.H, pitch.value, 1, dev.data_ptr(), t.W, t.H, t.W)  # a 1:1 copy
    ctx.resize_kernel_ms()
    return dev.cpu().numpy()


def test_tracker_equalize(vio, ctx):
    """the slot holds the oracle's equalised frame after upload + equalize, and after upload_resized + equalize"""
    torch = pytest.importorskip("torch")
    import resize_general_oracle as rgo
    W, H = 320, 160
    p = clahe_params(vio)
    cam = image("noise", 2 * W, 2 * H) // 4 + 96
    t = vio.Tracker(ctx, W, H, max_points=16, max_corners=16)
    img = image("narrow", W, H)
    t.upload(1, img)
    t.equalize(1, p)
    np.testing.assert_array_equal(_slot(vio, ctx, torch, t, 1), eo.clahe(img, 8, 8, 3.0))
    t.upload_resized(0, cam)
    t.equalize(0, p)
    small = rgo.resize_area_any(cam, W, H)
    assert small.shape == (H, W)
    np.testing.assert_array_equal(_slot(vio, ctx, torch, t, 0), eo.clahe(small, 8, 8, 3.0))
    t.equalize(0, vio.equalize_params(vio.VIO_EQ_NONE))  # nothing to do
    assert vio.lib().erp_tracker_equalize(t.h, 2, C.byref(p)) == -22
    assert vio.lib().erp_tracker_equalize(t.h, 0, C.byref(clahe_params(vio, 200, 8))) == -22
    t.sync()
    t.close()


@pytest.fixture(scope="module")
def low_contrast_sequence(synth):
    return [(96 + synth.render_erp(TW, TH, synth.rot_yaw_pitch(1.2 * f, 0.3 * f)) // 4).astype(np.uint8)
            for f in range(4)]


def _same(g, o, f):
    assert np.array_equal(g["ids"], o["ids"]), f
    assert np.array_equal(g["xy"], o["xy"]), f
    assert np.array_equal(g["track_count"], o["track_count"]) and np.array_equal(g["age"], o["age"]), f
    assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f


def test_frontend_equalize(vio, ctx, low_contrast_sequence):
    """a front end that equalises raw frames on the device = a plain front end fed the oracle's equalised frames"""
    prm = vio.default_frontend_params(seed=11)
    fe_eq = vio.Frontend(ctx, TW, TH, prm)
    fe_ref = vio.Frontend(ctx, TW, TH, prm)
    fe_eq.set_equalize(clahe_params(vio))
    carried = 0
    for f, raw in enumerate(low_contrast_sequence):
        eq = eo.clahe(raw, 8, 8, 3.0)
        assert np.count_nonzero(eq != raw) > raw.size // 2  # the equalisation really changes the frame
        g = fe_eq.track(raw)
        _same(g, fe_ref.track(eq), f)
        if f:
            carried += int((g["track_count"] > 0).sum())
    fe_eq.close()
    fe_ref.close()
    assert carried > 100  # features really are carried across frames


def test_frontend_equalize_off_again(vio, ctx, low_contrast_sequence):
    """after set_equalize(None) the front end is a plain one; a rejected setting leaves it as it was"""
    prm = vio.default_frontend_params(seed=11)
    fe = vio.Frontend(ctx, TW, TH, prm)
    fe_plain = vio.Frontend(ctx, TW, TH, prm)
    fe.set_equalize(clahe_params(vio))
    fe.set_equalize(None)
    assert vio.lib().erp_frontend_set_equalize(fe.h, C.byref(clahe_params(vio, 8, 8, float("nan")))) == -22
    n = 0
    for f, raw in enumerate(low_contrast_sequence[:2]):
        g = fe.track(raw)
        _same(g, fe_plain.track(raw), f)
        n += len(g["ids"])
    fe.set_equalize(vio.equalize_params(vio.VIO_EQ_NONE))
    _same(fe.track(low_contrast_sequence[2]), fe_plain.track(low_contrast_sequence[2]), 2)
    fe.close()
    fe_plain.close()
    assert n > 0
