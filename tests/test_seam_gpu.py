"""GPU parity of the seam wrap mode (VIO_SEAM_WRAP: tracking and detection across the ERP seam) against the
references of tests/seam_oracle.py, which run the unchanged CPU oracle on the frame continued periodically.

Bitwise wherever the reference computes at the frame's own coordinates (the right seam band, the interior,
detection, the pipeline on points at x >= 140); the left seam band, whose reference rounds every coordinate at another
column offset, within 7 x the spread two such references show against each other (tests/test_seam.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import seam_cases as sc
import seam_oracle as so

pytestmark = pytest.mark.gpu

# the largest spread of test_seam.py::test_klt_offset_spread over these inputs is 1.84e-4 px (f32 rounding of the
# coordinates at another offset, accumulated over <= 4 levels x 30 iterations); the kernel computes at a third
# offset (none), so it may differ from either by the same mechanism: 7 x that spread
LEFT_BAND_TOL = 1.3e-3


def padded(img, extra=24):
    """the same pixels in rows of W + extra bytes (the columns beyond the frame must never be read)"""
    big = np.full((img.shape[0], img.shape[1] + extra), 0x5A, np.uint8)
    big[:, :img.shape[1]] = img
    return big[:, :img.shape[1]]


def frames(W, H, flow):
    prev, curr = sc.pair(W, H, flow)
    return (padded(prev), padded(curr)) if W == 328 else (prev, curr)


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_klt_right_of_the_seam_bitwise(vio, gpu_ctx, W, H, flow):
    prev, curr = sc.pair(W, H, flow)
    pts = sc.right_band(W, H)
    klt = vio.default_klt_params()
    nxt, st, err = so.klt_track(prev, curr, pts, klt, 0, so.APRON)
    g = gpu_ctx.klt_track(*frames(W, H, flow), pts, klt, seam=vio.VIO_SEAM_WRAP)
    assert np.array_equal(g[1], st)
    assert np.array_equal(g[0], nxt)
    assert np.array_equal(g[2][st == 1], err[st == 1])
    assert ((g[0][:, 0] >= 0) & (g[0][:, 0] < W)).all()


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_klt_left_of_the_seam(vio, gpu_ctx, W, H, flow):
    prev, curr = sc.pair(W, H, flow)
    pts = sc.left_band(W, H)
    klt = vio.default_klt_params()
    nxt, st, _ = so.klt_track(prev, curr, pts, klt, so.APRON, so.APRON)
    g = gpu_ctx.klt_track(*frames(W, H, flow), pts, klt, seam=vio.VIO_SEAM_WRAP)
    assert np.array_equal(g[1], st)
    assert ((g[0][:, 0] >= 0) & (g[0][:, 0] < W)).all()
    ok = st == 1
    dx = np.abs(g[0][:, 0] - nxt[:, 0])[ok]
    dx = np.minimum(dx, W - dx)  # (a point within the tolerance of the seam may fold to either side)
    dy = np.abs(g[0][:, 1] - nxt[:, 1])[ok]
    print("left band", W, flow, float(dx.max()), float(dy.max()))
    assert max(dx.max(), dy.max()) <= LEFT_BAND_TOL


@pytest.mark.parametrize("W,H", sc.SIZES)
def test_klt_interior_invariance_bitwise(vio, gpu_ctx, W, H):
    """far from the seam WRAP is the flat tracker and the flat oracle; CUT is erp_klt_track for every point"""
    flow = sc.FLOWS[2]
    prev, curr = frames(W, H, flow)
    klt = vio.default_klt_params()
    pts = sc.interior(W, H)
    flat = gpu_ctx.klt_track(prev, curr, pts, klt)
    wrap = gpu_ctx.klt_track(prev, curr, pts, klt, seam=vio.VIO_SEAM_WRAP)
    o = oracle_lib.klt_track(*sc.pair(W, H, flow), pts, klt)
    assert o[1].mean() > 0.9
    for a in (flat, o):
        assert np.array_equal(wrap[1], a[1]) and np.array_equal(wrap[0], a[0])
        assert np.array_equal(wrap[2][o[1] == 1], a[2][o[1] == 1])
    every = np.concatenate([sc.corners(W, H), np.float32([[0, 0], [W - 0.1, H - 0.1], [-30, 50], [W + 40, 20]])])
    flat = gpu_ctx.klt_track(prev, curr, every, klt)
    cut = gpu_ctx.klt_track(prev, curr, every, klt, seam=vio.VIO_SEAM_CUT)
    for k in range(3):
        assert np.array_equal(flat[k], cut[k]), k


@pytest.mark.parametrize("W,H,mask,cap,md", sc.gftt_cases())
def test_gftt_bitwise(vio, gpu_ctx, W, H, mask, cap, md):
    img = sc.pair(W, H, sc.FLOWS[0])[0]
    m = sc.gftt_mask(W, H, mask)
    gi, gm = (padded(img), None if m is None else padded(m)) if W == 328 else (img, m)
    want = so.gftt(img, m, cap, sc.Q, md)
    got = gpu_ctx.gftt(gi, gm, cap, sc.Q, md, seam=vio.VIO_SEAM_WRAP)
    assert np.array_equal(got, want), (len(got), len(want))
    assert np.array_equal(gpu_ctx.gftt(gi, gm, cap, sc.Q, md, seam=vio.VIO_SEAM_CUT), gpu_ctx.gftt(gi, gm, cap, sc.Q, md))


def test_pipeline_bitwise(vio, gpu_ctx):
    from test_tracker_gpu import pipeline_oracle
    W, H = sc.SIZES[0]
    prev, curr = sc.pair(W, H, sc.FLOWS[2])
    pts = sc.pipeline_points(W, H)
    prm = vio.default_tracker_params(max_corners=200, seed=21)
    klt = vio.default_klt_params()
    nxt, st, kept, corners, crossing = so.pipeline_oracle(vio, prev, curr, pts, prm, klt)
    assert crossing >= 1 and ((corners[:, 0] < prm.min_dist) | (corners[:, 0] >= W - prm.min_dist)).any()
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
    t.upload(0, prev)
    t.upload(1, curr)
    t.set_points(pts)
    res = {}
    for mode in (vio.VIO_SEAM_WRAP, vio.VIO_SEAM_CUT, vio.VIO_SEAM_WRAP):  # and back again
        t.set_seam(mode)
        t.run(prm, klt)
        r = t.download()
        res[mode] = {k: v.copy() for k, v in r.items()}
        want = (nxt, st, kept, corners) if mode == vio.VIO_SEAM_WRAP else pipeline_oracle(vio, prev, curr, pts, prm, klt)
        for k, w in zip(("next", "status", "kept", "corners"), want):
            assert np.array_equal(res[mode][k], w), (mode, k)
    t.close()


def test_frontend_tracks_across_the_seam(vio, gpu_ctx):
    """six frames of the x-periodic texture rolled by d px per frame: a pure yaw of an ERP camera is exactly this
    roll, the true flow is (d, 0)"""
    W, H = sc.SIZES[0]
    d = 9
    base = sc.pair(W, H, sc.FLOWS[0])[0]
    seq = [np.roll(base, d * f, axis=1) for f in range(6)]
    prm = vio.default_frontend_params(seed=3)
    m = prm.boundary_margin
    klt = vio.default_klt_params()
    # the error the CPU oracle itself reaches on interior points of the same frames
    pts = sc.interior(W, H)
    e_oracle = 0.0
    for f in range(5):
        n, s, _ = oracle_lib.klt_track(seq[f], seq[f + 1], pts, klt)
        e_oracle = max(e_oracle, float(np.abs(n - (pts + np.float32([d, 0])))[s == 1].max()))
    print("front end: oracle error on interior points", e_oracle)
    crossed = {}
    for mode in (vio.VIO_SEAM_WRAP, vio.VIO_SEAM_CUT):
        fe = vio.Frontend(gpu_ctx, W, H, prm)
        fe.set_seam(mode)
        right, last, crossed[mode], worst = {}, {}, set(), 0.0
        for f, img in enumerate(seq):
            o = fe.track(img)
            assert ((o["xy"][:, 0] >= 0) & (o["xy"][:, 0] < W)).all()
            now = {}
            for i, xy, tc in zip(o["ids"], o["xy"], o["track_count"]):
                i, x = int(i), float(xy[0])
                now[i] = (xy, f)
                if x > W - m:
                    right[i] = int(tc)
                elif x < m and i in right:
                    assert tc > right[i]
                    crossed[mode].add(i)
            for i in crossed[mode]:  # the crossing ids follow the true flow, the step across the seam included
                if i in now and i in last and last[i][1] == f - 1:
                    ex = abs(float(now[i][0][0]) - float(so.fold_x(np.float32([last[i][0][0] + np.float32(d)]), W)[0]))
                    worst = max(worst, min(ex, W - ex), abs(float(now[i][0][1] - last[i][0][1])))
            last = now
        fe.close()
        if mode == vio.VIO_SEAM_WRAP:
            print("front end: crossing ids", len(crossed[mode]), "worst step error", worst)
            assert len(crossed[mode]) >= 1
            assert worst <= 2 * e_oracle
    assert not crossed[vio.VIO_SEAM_CUT]


def test_seam_check_failures_launch_nothing(vio, gpu_ctx):
    L = vio.lib()
    EINVAL = -22
    klt = vio.default_klt_params()

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    # 516 = 4 x 129 at max_level 3; a top level of 36 columns; W <= 2 min_dist; an unknown mode
    for (W, H) in ((516, 256), (144, 256)):
        img = np.zeros((H, W), np.uint8)
        pts, nxt = np.float32([[50, 100]]), np.full((1, 2), -7, np.float32)
        st, err = np.full(1, 9, np.uint8), np.zeros(1, np.float32)
        args = (gpu_ctx.h, ptr(img), ptr(img), W, H, W, ptr(pts), 1, ptr(nxt), ptr(st), ptr(err), C.byref(klt))
        assert L.erp_klt_track_seam(*args, vio.VIO_SEAM_WRAP) == EINVAL
        assert (nxt == -7).all() and st[0] == 9  # nothing was written
        assert L.erp_klt_track_seam(*args, 2) == EINVAL
        assert L.erp_klt_track_seam(*args, vio.VIO_SEAM_CUT) == 0
        t = vio.Tracker(gpu_ctx, W, H, max_points=8, max_corners=8)
        t.upload(0, img)
        t.upload(1, img)
        t.set_points(pts)
        t.set_seam(vio.VIO_SEAM_WRAP)
        prm = vio.default_tracker_params(max_corners=8)
        assert L.erp_tracker_run(t.h, C.byref(klt), C.byref(prm)) == EINVAL
        assert L.erp_tracker_set_seam(t.h, 2) == EINVAL
        t.set_seam(vio.VIO_SEAM_CUT)
        t.run(prm, klt)
        t.download()
        t.close()
        fe = vio.Frontend(gpu_ctx, W, H, vio.default_frontend_params())
        assert L.erp_frontend_set_seam(fe.h, vio.VIO_SEAM_WRAP) == EINVAL
        assert L.erp_frontend_set_seam(fe.h, vio.VIO_SEAM_CUT) == 0
        fe.close()
    img = np.zeros((64, 100), np.uint8)
    out, n = np.zeros((6400, 2), np.float32), C.c_int(-5)
    args = (gpu_ctx.h, ptr(img), None, 100, 64, 100, 0, C.c_double(0.01), C.c_double(50.0), ptr(out), C.byref(n))
    assert L.erp_gftt_seam(*args, vio.VIO_SEAM_WRAP) == EINVAL and n.value == -5  # W <= 2 min_dist
    assert L.erp_gftt_seam(*args, 7) == EINVAL
    assert L.erp_gftt_seam(*args, vio.VIO_SEAM_CUT) == 0 and n.value == 0
