"""GPU parity of the guided LK search (erp_klt_track_guess / erp_klt_track_rot, the tracker's and the front end's
predictions) against the NumPy restatement of tests/klt_guess_oracle.py, which tests/test_klt_guess.py pins to the C
oracle bit for bit.  Bitwise on next, status and err throughout; the rotation seed, whose atan2f / asinf are the
device's own, is read back (guess_out) and checked against the f64 predictor by angle."""
import ctypes as C

import numpy as np
import pytest

import guess_cases as gc
import klt_guess_oracle as ko
import seam_cases as sc
import seam_oracle as so
from test_seam_gpu import padded

pytestmark = pytest.mark.gpu

EINVAL = -22
# the seed of a point only has to land in LK's basin: 1e-5 rad is about 40 f32 ulps of pi, 0.006 px at W = 3840
ANGLE_BOUND = 1e-5
MODES = (ko.CUT, ko.WRAP)


def klt_params(vio, max_level=3, win=21):
    k = vio.default_klt_params()
    k.max_level, k.win = max_level, win
    return k


def dev(img):
    """the 328-wide frames go in padded rows"""
    return padded(img) if img.shape[1] == 328 else img


def few(a, n=300):
    """at most n rows of a, evenly spaced"""
    return a[::max(1, -(-len(a) // n))]


def assert_same(g, o, what=""):
    assert np.array_equal(g[1], o[1]), what
    assert np.array_equal(g[0], o[0]), what
    assert np.array_equal(g[2][o[1] == 1], o[2][o[1] == 1]), what


@pytest.mark.parametrize("name", list(gc.LARGE))
@pytest.mark.parametrize("W,H", gc.SIZES)
def test_explicit_guesses_bitwise(vio, gpu_ctx, W, H, name):
    prev, curr, pts, truth, R_seed = gc.large(name, W, H)
    pts, truth = few(pts), few(truth)
    guess = ko.predict(pts, R_seed, W, H)[0].astype(np.float32)
    for max_level, win in ((3, 21), (1, 21), (3, 9)):
        klt = klt_params(vio, max_level, win)
        for mode in MODES:
            o = ko.klt_track(prev, curr, pts, klt, guess, mode)
            g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, guess=guess)
            assert_same(g, o, (max_level, win, mode))
            if (max_level, win) == (3, 21):
                ok = (gc.error_px(g[0], truth, W) < 1.5) & (g[1] == 1)
                un = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode)
                lost = gc.error_px(un[0], truth, W) < 1.5
                print(name, W, "mode", mode, "within 1.5 px: guided", float(ok.mean()), "unguided", float(lost.mean()))
                assert lost.mean() <= 0.05
                if mode == ko.WRAP:
                    assert ok.mean() >= 0.90


@pytest.mark.parametrize("flow", sc.FLOWS)
@pytest.mark.parametrize("W,H", sc.SIZES)
def test_guess_equal_to_pts_is_the_unguided_tracker(vio, gpu_ctx, W, H, flow):
    prev, curr = sc.pair(W, H, flow)
    inside = np.concatenate([few(sc.corners(W, H), 250), np.float32([[0, 0], [W - 0.1, H - 0.1]])])
    # (a guess is folded into [0, W) in wrap mode, so there the identity is that of points inside the frame)
    every = np.concatenate([inside, np.float32([[-30, 50], [W + 40, 20]])])
    for max_level, win in ((3, 21), (1, 9)):
        klt = klt_params(vio, max_level, win)
        for mode in MODES:
            pts = inside if mode == ko.WRAP else every
            g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, guess=pts)
            u = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode)
            for k in range(3):
                assert np.array_equal(g[k], u[k]), (mode, k)
            assert_same(g, ko.klt_track(prev, curr, pts, klt, pts, mode), mode)


def seam_points(W, H, yaw_px):
    """points that an exact yaw of yaw_px takes onto the seam column (theta = +-pi, u == W or 0) and next to it"""
    ys = np.linspace(0.22 * H, 0.78 * H, 12, dtype=np.float32)
    xs = np.float32([W - yaw_px, W - yaw_px - 0.25, W - yaw_px + 0.25])
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.float32)


@pytest.mark.parametrize("name", list(gc.LARGE))
@pytest.mark.parametrize("W,H", gc.SIZES)
def test_rotation_seed(vio, gpu_ctx, synth, W, H, name):
    """measured on the device: the largest angle between the bearing of guess_out and R b of the f64 predictor is
    written to DESIGN.md 4.11 (the bound is 1e-5 rad)"""
    prev, curr, pts, truth, R_seed = gc.large(name, W, H)
    klt = vio.default_klt_params()
    cases = [(few(pts), R_seed)]
    if name == "yaw80":  # an exact yaw: the points of seam_points land on the seam itself
        R_yaw = synth.rot_yaw_pitch(80 * 360.0 / W, 0.0).astype(np.float32)
        cases.append((seam_points(W, H, 80), R_yaw))
    worst = 0.0
    for p, R in cases:
        d = ko.predict(p, R, W, H)[1]
        for mode in MODES:
            g = gpu_ctx.klt_track(dev(prev), dev(curr), p, klt, seam=mode, rot=R)
            used = g[3]
            ang = ko.angle_to(used, d, W, H)
            worst = max(worst, float(ang.max()))
            assert ang.max() <= ANGLE_BOUND, (mode, float(ang.max()))
            if mode == ko.WRAP:
                assert ((used[:, 0] >= 0) & (used[:, 0] < W)).all()
            else:
                assert ((used[:, 0] >= 0) & (used[:, 0] <= W)).all()
            assert_same(g, ko.klt_track(prev, curr, p, klt, used, mode), mode)
    print(name, W, "rotation seed: max angle to the f64 prediction", worst, "rad")
    if name == "yaw80":
        p, R = cases[1]
        used = gpu_ctx.klt_track(dev(prev), dev(curr), p, klt, seam=ko.WRAP, rot=R)[3]
        on_seam = used[::3, 0]  # the points taken onto theta = +-pi
        print("   seam column guesses", sorted(set(on_seam.tolist())))
        assert ((on_seam < 1e-2) | (on_seam > W - 1e-2)).all()


def test_bad_guesses_and_fold(vio, gpu_ctx):
    for (W, H) in sc.SIZES:
        prev, curr = sc.pair(W, H, sc.FLOWS[2])
        klt = vio.default_klt_params()
        pts = few(sc.corners(W, H), 120)
        good = pts + np.float32(sc.FLOWS[2])
        bads = np.float32([(np.nan, 100.0), (50.0, np.nan), (np.inf, 100.0), (-np.inf, 100.0), (50.0, np.inf),
                           (2.0 * W, 100.0), (-W - 1.0, 100.0), (50.0, 2.0 * H), (50.0, -H - 1.0), (-W, -H),
                           (np.nextafter(np.float32(2 * W), np.float32(0)), 100.0)])
        k = len(bads)
        for mode in MODES:
            g = good.copy()
            g[:k] = bads
            g[k:2 * k, 0] += np.float32(W)    # a turn to the right: WRAP folds it back, CUT loses the point
            g[2 * k:3 * k, 0] -= np.float32(W)
            got = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, guess=g)
            assert_same(got, ko.klt_track(prev, curr, pts, klt, g, mode), mode)
            un = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode)
            for q in range(3):  # the nine bad guesses: the unguided result, for those points only
                assert np.array_equal(got[q][:9], un[q][:9]), (mode, q)
        # and through the tracker, where the start positions can be read back
        t = vio.Tracker(gpu_ctx, W, H, max_points=256, max_corners=64)
        t.upload(0, dev(prev))
        t.upload(1, dev(curr))
        t.set_points(pts)
        prm = vio.default_tracker_params(max_corners=32, seed=5)
        for mode in MODES:
            t.set_seam(mode)
            t.set_guess(g)
            t.run(prm, klt)
            assert np.array_equal(t.download_guess(), ko.start_positions(pts, g, W, H, mode))
        t.close()


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_with_a_rotation(vio, gpu_ctx, mode):
    from test_tracker_gpu import pipeline_oracle
    W, H = sc.SIZES[0]
    prev, curr, _, _, R_seed = gc.large("yaw120_pitch10", W, H)
    pts = sc.pipeline_points(W, H)
    prm = vio.default_tracker_params(max_corners=200, seed=21)
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=1024)
    t.upload(0, prev)
    t.upload(1, curr)
    t.set_points(pts)
    t.set_seam(mode)
    t.set_rotation(R_seed)
    t.run(prm, klt)
    res = {k: v.copy() for k, v in t.download().items()}
    used = t.download_guess()
    t.run(prm, klt)  # no new prediction: the unguided pipeline
    res2 = {k: v.copy() for k, v in t.download().items()}
    with pytest.raises(vio.VioError):
        t.download_guess()
    t.close()
    ang = ko.angle_to(used, ko.predict(pts, R_seed, W, H)[1], W, H)
    assert ang.max() <= ANGLE_BOUND

    def oracle(guess):
        with ko.klt_step(lambda a, b, p, k, _m: ko.klt_track(a, b, p, k, guess, mode)[:3]):
            if mode == ko.WRAP:
                return so.pipeline_oracle(vio, prev, curr, pts, prm, klt)[:4]
            return pipeline_oracle(vio, prev, curr, pts, prm, klt)

    for r, want in ((res, oracle(used)), (res2, oracle(None))):
        for k, w in zip(("next", "status", "kept", "corners"), want):
            assert np.array_equal(r[k], w), (mode, k)
    # (the CUT restatement without a guess is the C oracle itself: the second run is the pipeline of old)
    if mode == ko.CUT:
        for k, w in zip(("next", "status", "kept", "corners"), pipeline_oracle(vio, prev, curr, pts, prm, klt)):
            assert np.array_equal(res2[k], w), k
    print("pipeline mode", mode, "kept with the rotation", int(res["kept"].sum()), "without", int(res2["kept"].sum()))
    assert res["kept"].sum() > 2 * res2["kept"].sum()


def rolled(W, H, d, n):
    base = sc.pair(W, H, sc.FLOWS[0])[0]
    return [np.roll(base, d * f, axis=1) for f in range(n)]


def test_frontend_cut_bitwise(vio, gpu_ctx, synth):
    """four frames of the texture rolled by 80 px per frame (a pure yaw is exactly this roll), the exact yaw
    predicted before each track; the guided front-end oracle starts from the device's own guesses"""
    W, H, d = 512, 256, 80
    seq = rolled(W, H, d, 4)
    R = synth.rot_yaw_pitch(d * 360.0 / W, 0.0).astype(np.float32)
    prm = vio.default_frontend_params(seed=3)
    klt = vio.default_klt_params()
    oracle = ko.guided_frontend(vio, W, H, prm, ko.CUT,
                                lambda a, b, p: gpu_ctx.klt_track(a, b, p, klt, seam=ko.CUT, rot=R)[3])
    fe = vio.Frontend(gpu_ctx, W, H, prm)
    tracked = []
    for img in seq:
        fe.predict_rotation(R)
        g, o = fe.track(img), oracle.track(img)
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g[k], o[k]), k
        tracked.append(o["num_tracked"])
    fe.close()
    print("front end CUT: tracked per frame", tracked)
    assert min(tracked[1:]) >= 30


def test_frontend_wrap_follows_a_fast_yaw(vio, gpu_ctx, synth):
    """the guided oracle keeps 72 of 72 frame-1 features with track_count 3 at frame 4 (tests/test_klt_guess.py), so
    the bar is the issue's 80 %"""
    W, H, d = 512, 256, 80
    seq = rolled(W, H, d, 4)
    R = synth.rot_yaw_pitch(d * 360.0 / W, 0.0).astype(np.float32)
    prm = vio.default_frontend_params(seed=3)
    share, crossed = {}, {}
    for guided in (True, False):
        fe = vio.Frontend(gpu_ctx, W, H, prm)
        fe.set_seam(vio.VIO_SEAM_WRAP)
        outs, last_x, last_tc, crossed[guided] = [], {}, {}, set()
        for img in seq:
            if guided:
                fe.predict_rotation(R)
            o = fe.track(img)
            assert ((o["xy"][:, 0] >= 0) & (o["xy"][:, 0] < W)).all()
            for i, xy, tc in zip(o["ids"].tolist(), o["xy"], o["track_count"].tolist()):
                if i in last_x and xy[0] < last_x[i] and tc > last_tc[i]:  # moved right by 80 px and came out left
                    crossed[guided].add(i)
                last_x[i], last_tc[i] = float(xy[0]), tc
            outs.append(o)
        fe.close()
        # every frame-1 feature stays outside the polar rows and the top / bottom margin (a pure yaw keeps its row),
        # and no mask is set
        first = set(outs[0]["ids"].tolist())
        alive = [i for i, tc in zip(outs[3]["ids"].tolist(), outs[3]["track_count"].tolist()) if i in first and tc == 3]
        share[guided] = len(alive) / len(first)
    print("front end WRAP: share alive at frame 4", share, "ids across the seam", len(crossed[True]))
    assert len(crossed[True]) >= 1
    assert share[True] >= 0.8
    assert share[False] == 0.0


def test_errors_launch_nothing(vio, gpu_ctx):
    from test_tracker_gpu import pipeline_oracle
    L = vio.lib()
    W, H = sc.SIZES[0]
    prev, curr = sc.pair(W, H, sc.FLOWS[0])
    klt = vio.default_klt_params()
    pts = sc.pipeline_points(W, H)
    n = len(pts)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def refused(rc, who):
        assert rc == EINVAL, (who, rc)
        assert who.encode() in L.vio_ctx_last_error(gpu_ctx.h), (who, L.vio_ctx_last_error(gpu_ctx.h))

    nxt, st, err = np.full((n, 2), -7, np.float32), np.full(n, 9, np.uint8), np.zeros(n, np.float32)
    used = np.full((n, 2), -7, np.float32)
    R = np.eye(3, dtype=np.float32).reshape(9)
    not_rot = [np.float32(1.01) * R, np.float32([1, 0, 0, 0, 1, 0, 0, 0, -1]), np.full(9, np.nan, np.float32),
               np.zeros(9, np.float32)]
    head = (gpu_ctx.h, ptr(prev), ptr(curr), W, H, W, ptr(pts))
    tail = (ptr(nxt), ptr(st), ptr(err))
    for bad in not_rot:
        refused(L.erp_klt_track_rot(*head, n, ptr(bad), *tail, ptr(used), C.byref(klt), ko.CUT), "erp_klt_track_rot")
    refused(L.erp_klt_track_rot(*head, n, None, *tail, ptr(used), C.byref(klt), ko.CUT), "erp_klt_track_rot")
    refused(L.erp_klt_track_rot(*head, n, ptr(R), *tail, ptr(used), C.byref(klt), 2), "erp_klt_track_rot")
    refused(L.erp_klt_track_guess(*head, None, n, *tail, C.byref(klt), ko.CUT), "erp_klt_track_guess")
    refused(L.erp_klt_track_guess(*head, ptr(pts), n, *tail, C.byref(klt), 7), "erp_klt_track_guess")
    # WRAP on a size erp_seam_check refuses (516 = 4 x 129 at max_level 3)
    img = np.zeros((256, 516), np.uint8)
    odd = (gpu_ctx.h, ptr(img), ptr(img), 516, 256, 516, ptr(pts))
    assert vio.lib().erp_seam_check(516, 256, 21, 3, 0.0) == EINVAL
    refused(L.erp_klt_track_rot(*odd, n, ptr(R), *tail, ptr(used), C.byref(klt), ko.WRAP), "erp_klt_track_rot")
    refused(L.erp_klt_track_guess(*odd, ptr(pts), n, *tail, C.byref(klt), ko.WRAP), "erp_klt_track_guess")
    assert (nxt == -7).all() and (st == 9).all() and (used == -7).all()  # nothing was written

    prm = vio.default_tracker_params(max_corners=100, seed=9)
    t = vio.Tracker(gpu_ctx, W, H, max_points=1024, max_corners=256)
    t.upload(0, prev)
    t.upload(1, curr)
    t.set_points(pts)
    for bad in not_rot:
        refused(L.erp_tracker_set_rotation(t.h, ptr(bad)), "erp_tracker_set_rotation")
    refused(L.erp_tracker_set_rotation(t.h, None), "erp_tracker_set_rotation")
    refused(L.erp_tracker_set_guess(t.h, ptr(pts), n - 1), "erp_tracker_set_guess")
    refused(L.erp_tracker_set_guess(t.h, ptr(pts), n + 1), "erp_tracker_set_guess")
    refused(L.erp_tracker_set_guess(t.h, None, n), "erp_tracker_set_guess")
    refused(L.erp_tracker_download_guess(t.h, ptr(used)), "erp_tracker_download_guess")  # nothing ran yet
    t.run(prm, klt)  # none of the refused calls left a prediction behind
    res = t.download()
    for k, w in zip(("next", "status", "kept", "corners"), pipeline_oracle(vio, prev, curr, pts, prm, klt)):
        assert np.array_equal(res[k], w), k
    t.close()

    t = vio.Tracker(gpu_ctx, 516, 256, max_points=64, max_corners=256)
    t.upload(0, img)
    t.upload(1, img)
    t.set_points(pts[:8])
    t.set_seam(vio.VIO_SEAM_WRAP)
    t.set_rotation(R)
    refused(L.erp_tracker_run(t.h, C.byref(klt), C.byref(prm)), "erp_tracker_run")
    t.close()

    fe = vio.Frontend(gpu_ctx, W, H, vio.default_frontend_params(seed=3))
    for bad in not_rot:
        refused(L.erp_frontend_predict_rotation(fe.h, ptr(bad)), "erp_frontend_predict_rotation")
    refused(L.erp_frontend_predict_rotation(fe.h, None), "erp_frontend_predict_rotation")
    import frontend_oracle
    oracle = frontend_oracle.FrontendOracle(vio, W, H, vio.default_frontend_params(seed=3))
    for img2 in (prev, curr):
        g, o = fe.track(img2), oracle.track(img2)
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g[k], o[k]), k
    fe.close()
