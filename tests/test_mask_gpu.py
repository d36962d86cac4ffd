"""GPU parity of the region masks (csrc/mask.hip and their use in the tracker pipeline and the front end) against
tests/mask_oracle.py — bitwise: the stand-alone builds at sizes that straddle the 32-pixel words, the builds through
a warp, the tracker pipeline and the front end with a mask, and the way back to the maskless pipeline."""
import ctypes as C

import numpy as np
import pytest

import equalize_oracle as eo
import mask_oracle as mo
import oracle_lib
import warp_oracle as wo

pytestmark = pytest.mark.gpu

BORDERS = (mo.X_CLAMP, mo.X_WRAP)
RADII = (0, 1, 2, 5, 31, 32, 40, 255)
# dW in {32, 37, 53, 65, 97}: a whole word, a partial one, two words and one bit, three words and one bit
SHAPES = [((53, 37), (53, 37)), ((96, 40), (32, 20)), ((101, 67), (37, 23)), ((200, 16), (65, 8)), ((97, 9), (97, 9))]


def source_masks(sW, sH):
    """name -> (sH, sW) u8, nonzero = usable (any nonzero value counts)"""
    rng = np.random.default_rng(sW * 1000 + sH)
    y, x = np.mgrid[0:sH, 0:sW]
    blobs = np.full((sH, sW), 255, np.uint8)
    blobs[((x - sW * 0.4) / (sW * 0.12)) ** 2 + ((y - sH * 0.5) / (sH * 0.3)) ** 2 <= 1] = 0
    blobs[((((x + sW // 2) % sW) - sW * 0.5) / (sW * 0.06)) ** 2 + ((y - sH * 0.3) / (sH * 0.2)) ** 2 <= 1] = 0  # seam
    corners = np.full((sH, sW), 255, np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 0
    return {"all usable": rng.integers(1, 256, (sH, sW)).astype(np.uint8),
            "all excluded": np.zeros((sH, sW), np.uint8),
            "bernoulli": np.where(rng.random((sH, sW)) < 0.01, 0, rng.integers(1, 256, (sH, sW))).astype(np.uint8),
            "blobs": blobs, "corners": corners}


@pytest.mark.parametrize("src,dst", SHAPES)
def test_build_bitwise_vs_oracle(vio, gpu_ctx, src, dst):
    (sW, sH), (dW, dH) = src, dst
    for name, m in source_masks(sW, sH).items():
        reduced = mo.reduce(m, dW, dH)
        if name == "blobs":
            assert (reduced[:, 0] == 0).any() and (reduced[:, -1] == 0).any() and (reduced == 255).any()
        for r in RADII:
            for border in BORDERS:
                got = gpu_ctx.mask_build(m, dW, dH, vio.mask_params(r, border))
                np.testing.assert_array_equal(got, mo.erode(reduced, r, border), err_msg=f"{name} r={r} border={border}")
    assert gpu_ctx.mask_kernel_ms() > 0


def test_build_honours_the_host_stride(vio, gpu_ctx):
    big = np.zeros((67, 130), np.uint8)  # the columns beyond the mask are excluded: they must not be read
    m = source_masks(101, 67)["bernoulli"]
    big[:, :101] = m
    np.testing.assert_array_equal(gpu_ctx.mask_build(big[:, :101], 37, 23, vio.mask_params(1, mo.X_WRAP)),
                                  mo.build(m, 37, 23, 1, mo.X_WRAP))


def test_build_device_unaligned(vio, gpu_ctx):
    """device buffers at an odd source offset with a stride of sW + 3; the destination's padding is not written"""
    torch = pytest.importorskip("torch")
    (sW, sH), (dW, dH) = (101, 67), (37, 23)
    m = source_masks(sW, sH)["bernoulli"]
    stride, off, dstride, doff = sW + 3, 1, dW + 5, 3
    host = np.zeros((sH, stride), np.uint8)  # padding: excluded, must not be read
    host[:, :sW] = m
    d_src = torch.zeros(off + host.size + 16, dtype=torch.uint8, device="cuda:0")
    d_src[off:off + host.size] = torch.from_numpy(host.reshape(-1)).to("cuda:0")
    d_dst = torch.full((doff + dH * dstride,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.mask_build_device(d_src.data_ptr() + off, sW, sH, stride, dW, dH, vio.mask_params(2, mo.X_WRAP),
                              d_dst.data_ptr() + doff, dstride)
    assert gpu_ctx.mask_kernel_ms() > 0  # waits for the launches
    out = d_dst.cpu().numpy()
    assert (out[:doff] == 0xA5).all()
    out = out[doff:].reshape(dH, dstride)
    np.testing.assert_array_equal(out[:, :dW], mo.build(m, dW, dH, 2, mo.X_WRAP))
    assert (out[:, dW:] == 0xA5).all()


# ---- through a warp ----

R_WARP = wo.rot_y(0.31) @ wo.rot_x(0.17)


def test_build_warped_rotated_erp(vio, gpu_ctx):
    """80 x 48 -> 64 x 32 under a yaw / pitch rotation, WRAP + REPLICATE, a random source mask"""
    sW, sH, dW, dH = 80, 48, 64, 32
    mx, my = vio.warp_map_erp(sW, sH, dW, dH, R_WARP)
    m = np.where(np.random.default_rng(8).random((sH, sW)) < 0.05, 0, 255).astype(np.uint8)
    m[:, 0] = 0  # the seam column: reached through the wrapped tap
    w = gpu_ctx.warp_create(mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE)
    want = mo.warp_usable(m, mx, my, sW, sH, wo.X_WRAP, wo.Y_REPLICATE)
    assert (want == 0).any() and (want == 255).any()
    np.testing.assert_array_equal(w.mask_build(m), want)
    np.testing.assert_array_equal(w.mask_build(None), np.full((dH, dW), 255, np.uint8))  # nothing is outside
    np.testing.assert_array_equal(w.mask_build(m, params=vio.mask_params(1, mo.X_WRAP)), mo.erode(want, 1, mo.X_WRAP))
    w.close()


@pytest.mark.parametrize("bx", [wo.X_CONSTANT, wo.X_WRAP])
@pytest.mark.parametrize("by", [wo.Y_CONSTANT, wo.Y_REPLICATE])
def test_build_warped_random_maps(vio, gpu_ctx, bx, by):
    """coordinates uniform in [-3, S + 3] with integers, ties, both borders, far-outside and non-finite values:
    taps outside the source under every pair of border modes; 70 columns: two words and a partial one"""
    sW, sH, dW, dH = 37, 23, 70, 11
    rng = np.random.default_rng(20 + bx + by)
    maps = []
    for S in (sW, sH):
        v = rng.uniform(-3, S + 3, dW * dH).astype(np.float32)
        sp = wo.special_coordinates(S)
        v[rng.choice(v.size, sp.size, replace=False)] = sp
        maps.append(v.reshape(dH, dW))
    m = np.where(rng.random((sH, sW)) < 0.1, 0, rng.integers(1, 256, (sH, sW))).astype(np.uint8)
    w = gpu_ctx.warp_create(maps[0], maps[1], sW, sH, bx, by)
    for src in (None, m):
        want = mo.warp_usable(src, maps[0], maps[1], sW, sH, bx, by)
        assert (want == 0).any() and (want == 255).any()
        np.testing.assert_array_equal(w.mask_build(src), want)
    w.close()


def fisheye_maps(vio, dW, dH, circle):
    return vio.warp_map_fisheye(wo.dual_fisheye(80.0, circle), dW, dH, wo.rot_y(0.1234) @ wo.rot_x(0.0567))


def test_build_warped_fisheye_null_mask(vio, gpu_ctx):
    """two lenses, theta_max 80 degrees, CONSTANT borders, no source mask: the warp's holes and rim"""
    mx, my = fisheye_maps(vio, 64, 32, 32)
    assert np.isnan(mx).any()
    w = gpu_ctx.warp_create(mx, my, 64, 32, wo.X_CONSTANT, wo.Y_CONSTANT, 200)
    want = mo.warp_usable(None, mx, my, 64, 32, wo.X_CONSTANT, wo.Y_CONSTANT)
    assert (want[np.isnan(mx)] == 0).all() and (want == 255).any()
    np.testing.assert_array_equal(w.mask_build(None), want)
    w.close()


def test_build_warped_supersampled(vio, gpu_ctx):
    """a 128 x 64 warp reduced to 64 x 32, r = 2"""
    mx, my = fisheye_maps(vio, 128, 64, 32)
    m = np.where(np.random.default_rng(9).random((32, 64)) < 0.02, 0, 255).astype(np.uint8)
    w = gpu_ctx.warp_create(mx, my, 64, 32, wo.X_CONSTANT, wo.Y_CONSTANT)
    for src in (None, m):
        for border in BORDERS:
            want = mo.build_warped(src, mx, my, 64, 32, wo.X_CONSTANT, wo.Y_CONSTANT, 64, 32, 2, border)
            assert (want == 0).any() and (want == 255).any()
            np.testing.assert_array_equal(w.mask_build(src, 64, 32, vio.mask_params(2, border)), want)
    L, p, out = vio.lib(), vio.mask_params(), np.zeros((64, 129), np.uint8)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.erp_mask_build_warped(w.h, None, 0, 129, 64, C.byref(p), ptr, 129) == -38  # a warp smaller than the mask
    assert L.erp_mask_build_warped(w.h, None, 0, 64, 32, C.byref(p), ptr, 63) == -22
    assert L.erp_mask_build_warped(w.h, ptr, 63, 64, 32, C.byref(p), ptr, 64) == -22   # stride < the source's width
    w.close()


# ---- the tracker pipeline ----

W, H = 960, 480


def rig_mask(W, H):
    """an operator: an ellipse of about 12 % of the frame, low centre, reaching into the textured band; and a pole
    across the seam"""
    y, x = np.mgrid[0:H, 0:W]
    m = np.full((H, W), 255, np.uint8)
    m[((x - W * 0.5) / (W * 0.23)) ** 2 + ((y - H * 0.84) / (H * 0.17)) ** 2 <= 1] = 0
    m[int(H * 0.3):int(H * 0.62), :int(W * 0.04)] = 0
    m[int(H * 0.3):int(H * 0.62), W - int(W * 0.03):] = 0
    return m


def base_region(W, H, margin=20, polar=0.15):
    return mo.region_mask(W, H, margin, polar)


@pytest.fixture(scope="module")
def pair(synth):
    return synth.config1(W, H)


@pytest.fixture(scope="module")
def rig(vio):
    m = rig_mask(W, H)
    return m, vio.mask_params(10, mo.X_WRAP), mo.build(m, W, H, 10, mo.X_WRAP)


def run_pipeline(vio, ctx, a, b, pts, prm, klt, mask=None, params=None, also_cleared=False, max_corners=1024):
    t = vio.Tracker(ctx, a.shape[1], a.shape[0], max_points=1024, max_corners=max_corners)
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    if mask is not None:
        t.set_mask(mask, params)
    t.run(prm, klt)
    res = [t.download()]
    fb = t.gftt_fallbacks()
    if also_cleared:
        t.set_mask(None)
        t.run(prm, klt)
        res.append(t.download())
    t.close()
    return res, fb


def same_pipeline(res, nxt, st, kept, corners):
    assert np.array_equal(res["status"], st)
    assert np.array_equal(res["next"], nxt)
    assert np.array_equal(res["kept"], kept)
    assert np.array_equal(res["corners"], corners)


def test_pipeline_masked_bitwise(vio, gpu_ctx, pair, rig):
    from test_tracker_gpu import pipeline_oracle
    a, b, _ = pair
    mask, params, usable = rig
    pts0 = oracle_lib.gftt(a, base_region(W, H), 300, float(np.float32(0.01)), 30.0)
    rng = np.random.default_rng(2)
    bad = np.stack([rng.uniform(30, 930, 20), rng.uniform(80, 400, 20)], -1).astype(np.float32)
    pts = np.concatenate([pts0, bad])
    prm = vio.default_tracker_params(max_corners=300, seed=77)
    klt = vio.default_klt_params()
    nxt, st, kept, corners, dropped = mo.pipeline_oracle_masked(vio, a, b, pts, prm, klt, usable)
    plain = pipeline_oracle(vio, a, b, pts, prm, klt)
    # the mask really bites (on the oracle alone)
    assert kept.sum() > 150 and dropped >= 10
    assert mo.usable_at(usable, corners[:, 0], corners[:, 1]).all() and len(corners) > 0
    assert not np.array_equal(corners, plain[3])
    res, _ = run_pipeline(vio, gpu_ctx, a, b, pts, prm, klt, mask, params, also_cleared=True)
    same_pipeline(res[0], nxt, st, kept, corners)
    same_pipeline(res[1], *plain)  # set_mask(None): the maskless pipeline again


@pytest.mark.parametrize("npts,max_corners,quality", [(300, 1000, 0.01), (300, 4, 0.01)])
def test_pipeline_masked_presel_cases_bitwise(vio, gpu_ctx, pair, rig, npts, max_corners, quality):
    """the presort's prefix knows nothing of the mask: a fallback may be taken, the bits may not differ"""
    a, b, _ = pair
    mask, params, usable = rig
    pts = oracle_lib.gftt(a, base_region(W, H), 300, float(np.float32(0.01)), 30.0)[:npts]
    prm = vio.default_tracker_params(max_corners=max_corners, seed=5)
    prm.quality = float(np.float32(quality))
    klt = vio.default_klt_params()
    res, fb = run_pipeline(vio, gpu_ctx, a, b, pts, prm, klt, mask, params)
    nxt, st, kept, corners, _ = mo.pipeline_oracle_masked(vio, a, b, pts, prm, klt, usable)
    same_pipeline(res[0], nxt, st, kept, corners)
    assert fb[1] == 0 and fb[0] in (0, 1)


@pytest.mark.parametrize("border", BORDERS)
def test_pipeline_masked_odd_size(vio, synth, gpu_ctx, border):
    """333 x 171 (partial last word, partial tiles), margin 8, min_dist 6, random blobs, r = 3"""
    Wo, Ho = 333, 171
    a, b, _ = synth.config1(Wo, Ho)
    rng = np.random.default_rng(12)
    y, x = np.mgrid[0:Ho, 0:Wo]
    mask = np.full((Ho, Wo), 255, np.uint8)
    for _ in range(9):
        cx, cy, rx, ry = rng.uniform(0, Wo), rng.uniform(30, Ho - 30), rng.uniform(6, 30), rng.uniform(5, 16)
        mask[((((x - cx + Wo // 2) % Wo) - Wo // 2) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1] = 0
    usable = mo.build(mask, Wo, Ho, 3, border)
    prm = vio.default_tracker_params(max_corners=80, seed=9)
    prm.boundary_margin, prm.min_dist = 8, 6.0
    klt = vio.default_klt_params()
    pts = oracle_lib.gftt(a, base_region(Wo, Ho, 8), 80, float(np.float32(0.01)), 6.0)
    nxt, st, kept, corners, dropped = mo.pipeline_oracle_masked(vio, a, b, pts, prm, klt, usable)
    assert kept.sum() > 20 and dropped > 0 and len(corners) > 0
    res, _ = run_pipeline(vio, gpu_ctx, a, b, pts, prm, klt, mask, vio.mask_params(3, border), max_corners=128)
    same_pipeline(res[0], nxt, st, kept, corners)


def test_get_mask(vio, gpu_ctx):
    """the plane after set_mask (camera resolution, a non-integer reduce), set_mask_device and set_mask_warped;
    all 255 after a clear; a failed call leaves the previous mask in place"""
    torch = pytest.importorskip("torch")
    TW, TH = 160, 80
    t = vio.Tracker(gpu_ctx, TW, TH, max_points=16, max_corners=16)
    full = np.full((TH, TW), 255, np.uint8)
    np.testing.assert_array_equal(t.get_mask(), full)
    cam = source_masks(333, 171)["blobs"]
    t.set_mask(cam, vio.mask_params(2, mo.X_WRAP))
    want = mo.build(cam, TW, TH, 2, mo.X_WRAP)
    assert (want == 0).any() and (want == 255).any()
    np.testing.assert_array_equal(t.get_mask(), want)
    # rejected calls: the mask stays
    L, ptr = vio.lib(), cam.ctypes.data_as(C.c_void_p)
    assert L.erp_tracker_set_mask(t.h, ptr, 333, 171, 333, C.byref(vio.mask_params(256))) == -22
    assert L.erp_tracker_set_mask(t.h, ptr, 333, 171, 333, C.byref(vio.mask_params(1, 2))) == -22
    assert L.erp_tracker_set_mask(t.h, ptr, 333, 171, 332, C.byref(vio.mask_params())) == -22
    assert L.erp_tracker_set_mask(t.h, ptr, 159, 171, 333, C.byref(vio.mask_params())) == -38  # smaller than the frame
    assert L.erp_tracker_set_mask(t.h, ptr, 333, 171, 333, None) == -22
    np.testing.assert_array_equal(t.get_mask(), want)
    # a device mask at the tracker's size
    m = source_masks(TW, TH)["bernoulli"]
    d = torch.from_numpy(m).to("cuda:0")
    torch.cuda.synchronize()
    t.set_mask_device(d.data_ptr(), TW, TH, TW, vio.mask_params(1, mo.X_CLAMP))
    np.testing.assert_array_equal(t.get_mask(), mo.build(m, TW, TH, 1, mo.X_CLAMP))
    # through a warp larger than the tracker
    mx, my = fisheye_maps(vio, 200, 100, 64)
    w = gpu_ctx.warp_create(mx, my, 128, 64, wo.X_CONSTANT, wo.Y_CONSTANT)
    src = np.where(np.random.default_rng(10).random((64, 128)) < 0.01, 0, 255).astype(np.uint8)
    for s in (None, src):
        t.set_mask_warped(w, s, vio.mask_params(1, mo.X_WRAP))
        want = mo.build_warped(s, mx, my, 128, 64, wo.X_CONSTANT, wo.Y_CONSTANT, TW, TH, 1, mo.X_WRAP)
        assert (want == 0).any() and (want == 255).any()
        np.testing.assert_array_equal(t.get_mask(), want)
    small = gpu_ctx.warp_create(mx[:50, :100], my[:50, :100], 128, 64)
    assert L.erp_tracker_set_mask_warped(t.h, small.h, None, 0, C.byref(vio.mask_params())) == -38
    other = vio.Context(0)
    foreign = other.warp_create(mx, my, 128, 64)
    assert L.erp_tracker_set_mask_warped(t.h, foreign.h, None, 0, C.byref(vio.mask_params())) == -22
    foreign.close()
    other.close()
    np.testing.assert_array_equal(t.get_mask(), want)
    t.set_mask(None)
    np.testing.assert_array_equal(t.get_mask(), full)
    small.close()
    w.close()
    t.close()


# ---- the front end ----

def same_features(g, o, f):
    assert np.array_equal(g["ids"], o["ids"]), f
    assert np.array_equal(g["xy"], o["xy"]), f
    assert np.array_equal(g["track_count"], o["track_count"]) and np.array_equal(g["age"], o["age"]), f
    assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f


@pytest.fixture(scope="module")
def sequence(synth):
    return [synth.render_erp(W, H, synth.rot_yaw_pitch(1.2 * f, 0.3 * f)) for f in range(6)]


@pytest.mark.parametrize("clustered", [1, 0])
def test_frontend_masked_sequence(vio, gpu_ctx, sequence, rig, clustered):
    mask, params, usable = rig
    prm = vio.default_frontend_params(seed=11)
    prm.remove_clustered = clustered
    fe = vio.Frontend(gpu_ctx, W, H, prm)
    fe.set_mask(mask, params)
    orc = mo.MaskedFrontendOracle(vio, W, H, prm, usable)
    carried = dropped = 0
    for f, img in enumerate(sequence):
        o = orc.track(img)
        dropped += orc.mask_dropped
        assert mo.usable_at(usable, o["xy"][:, 0], o["xy"][:, 1]).all(), f  # no feature on an excluded pixel
        if f:
            carried += int((o["track_count"] > 0).sum())
        same_features(fe.track(img), o, f)
    fe.close()
    assert carried > 300 and dropped >= 5  # (on the oracle alone) features are carried, the mask term drops some


def test_frontend_masked_warped_equalized(vio, synth, gpu_ctx):
    """set_mask_warped + track_warped + set_equalize on a 480 x 240 dual-fisheye warp (theta_max 80 degrees: holes
    between the lenses) = the masked oracle on the oracle's warped, equalised frames"""
    FW, FH = 480, 240
    mx, my = fisheye_maps(vio, FW, FH, FH)
    w = gpu_ctx.warp_create(mx, my, FW, FH, wo.X_CONSTANT, wo.Y_CONSTANT)
    usable = mo.build_warped(None, mx, my, FW, FH, wo.X_CONSTANT, wo.Y_CONSTANT, FW, FH, 3, mo.X_CLAMP)
    assert 0.05 < (usable == 0).mean() < 0.6
    prm = vio.default_frontend_params(seed=11)
    fe = vio.Frontend(gpu_ctx, FW, FH, prm)
    fe.set_mask_warped(w, None, vio.mask_params(3, mo.X_CLAMP))
    fe.set_equalize(vio.equalize_params(vio.VIO_EQ_CLAHE, 8, 8, 3.0))
    orc = mo.MaskedFrontendOracle(vio, FW, FH, prm, usable)
    carried = 0
    for f in range(3):
        lens = synth.render_erp(FW, FH, synth.rot_yaw_pitch(0.6 * f, 0.2 * f))  # stands for the lens image
        o = orc.track(eo.clahe(wo.remap_grey(lens, mx, my, wo.X_CONSTANT, wo.Y_CONSTANT, 0), 8, 8, 3.0))
        assert mo.usable_at(usable, o["xy"][:, 0], o["xy"][:, 1]).all(), f
        if f:
            carried += int((o["track_count"] > 0).sum())
        same_features(fe.track_warped(w, lens), o, f)
    fe.close()
    w.close()
    assert carried > 20
