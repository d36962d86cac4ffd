"""GPU parity of the round-trip check (erp_klt_track_fb, erp_tracker_set_fb, erp_frontend_set_fb) against the reference
of tests/klt_fb_oracle.py: two calls of the guided NumPy restatement, which tests/test_klt_guess.py pins to the C
oracle, and the distance test in f32.  Bitwise on all six outputs: err where the final status is 1, back and fb_d2
where the backward search ended inside the frame (fb_state PASS or TOO_FAR)."""
import ctypes as C

import numpy as np
import pytest

import fb_cases as fc
import guess_cases as gc
import klt_fb_oracle as fbo
import klt_guess_oracle as ko
import seam_cases as sc
import seam_oracle as so
from test_seam_gpu import padded

pytestmark = pytest.mark.gpu

EINVAL = -22
MODES = (ko.CUT, ko.WRAP)
KLTS = ((3, 21), (1, 21), (3, 9))
DISTS = (0.5, 0.0, 2.0)
PAIRS = {"occluded": fc.occluded, "plain": fc.plain}


def klt_params(vio, max_level=3, win=21):
    k = vio.default_klt_params()
    k.max_level, k.win = max_level, win
    return k


def dev(img):
    """the 328-wide frames go in padded rows"""
    return padded(img) if img.shape[1] == 328 else img


def assert_same(g, o, what=""):
    """g, o: (next, status, err, back, fb_state, fb_d2)"""
    assert np.array_equal(g[4], o[4]), (what, "fb_state")
    assert np.array_equal(g[1], o[1]), (what, "status")
    assert np.array_equal(g[0], o[0]), (what, "next")
    assert np.array_equal(g[2][o[1] == 1], o[2][o[1] == 1]), (what, "err")
    ran = (o[4] == fbo.PASS) | (o[4] == fbo.TOO_FAR)
    assert np.array_equal(g[3][ran], o[3][ran]), (what, "back")
    assert np.array_equal(g[5][ran], o[5][ran]), (what, "fb_d2")
    # where the backward search was not run, and where it lost the point: the header's zeros
    assert not g[3][o[4] == fbo.NOT_RUN].any() and not g[5][~ran].any(), (what, "zeros")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("W,H", fc.SIZES)
def test_one_shot_bitwise(vio, gpu_ctx, W, H, pair, mode):
    prev, curr = PAIRS[pair](W, H)
    pts = fc.points(W, H)
    for max_level, win in KLTS:
        klt = klt_params(vio, max_level, win)
        trip = fbo.round_trip(prev, curr, pts, klt, None, mode)
        for dist in DISTS:
            o = fbo.judge(trip, dist)
            g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, fb=vio.default_fb_params(dist))
            assert_same(g, o, (max_level, win, dist))
            if dist == 0.5 and (max_level, win) == (3, 21):
                print(pair, W, "mode", mode, "found", int((o[4] != 0).sum()), "pass", int(o[1].sum()),
                      "back lost, too far", fbo.counts(o[4])[1:])
                # the cases are no empty ones: points pass, and on the occluded pair the check rejects some
                assert o[1].sum() > 0 and (pair == "plain" or (o[4] == fbo.TOO_FAR).sum() >= 20)


@pytest.mark.parametrize("W,H", fc.SIZES)
def test_seam_band_and_points_outside_the_frame(vio, gpu_ctx, W, H):
    """tracks that cross the seam (the short way round in the test), and in CUT two points outside the frame, whose
    previous position is a guess like any other for the way back"""
    prev, curr = fc.occluded(W, H)
    klt = vio.default_klt_params()
    band = sc.right_band(W, H)
    assert len(band) >= 10
    for mode in MODES:
        pts = band if mode == ko.WRAP else np.concatenate([band, np.float32([[-30, 50], [W + 40, 20]])])
        trip = fbo.round_trip(prev, curr, pts, klt, None, mode)
        for dist in DISTS:
            o = fbo.judge(trip, dist)
            g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, fb=vio.default_fb_params(dist))
            assert_same(g, o, (mode, dist))
        if mode == ko.WRAP:  # tracks cross the seam and come back across it
            o = fbo.judge(trip, 0.5)
            crossed = (o[1] == 1) & (o[0][:, 0] < pts[:, 0])
            print(W, "WRAP: of", len(pts), "band points", int(o[1].sum()), "pass,", int(crossed.sum()), "across the seam")
            assert crossed.sum() >= 1


def test_no_points_and_nothing_found(vio, gpu_ctx):
    W, H = fc.SIZES[0]
    prev, curr = fc.occluded(W, H)
    pts = fc.points(W, H)
    klt = vio.default_klt_params()
    fb = vio.default_fb_params()
    flat = np.full_like(prev, 90)
    for mode in MODES:
        g = gpu_ctx.klt_track(prev, curr, pts[:0], klt, seam=mode, fb=fb)
        assert [len(a) for a in g] == [0] * 6
        # a flat first frame has no texture to follow: every point is forward-lost and nothing is tracked back
        g = gpu_ctx.klt_track(flat, curr, pts, klt, seam=mode, fb=fb)
        o = fbo.fb_track(flat, curr, pts, klt, None, mode, 0.5)
        assert (o[4] == fbo.NOT_RUN).all() and not o[1].any()
        assert_same(g, o, mode)
        assert not g[3].any() and not g[5].any()
        # a flat second frame: whatever the reference makes of it
        assert_same(gpu_ctx.klt_track(prev, flat, pts, klt, seam=mode, fb=fb),
                    fbo.fb_track(prev, flat, pts, klt, None, mode, 0.5), (mode, "flat curr"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", fc.SIZES)
def test_identity_on_the_device(vio, gpu_ctx, W, H, mode):
    """the fused instance is the composition of the existing entry points: its backward half equals
    erp_klt_track_guess(curr, prev, next[found], pts[found]), its forward half the unchecked call"""
    prev, curr = fc.occluded(W, H)
    pts = fc.points(W, H)
    klt = vio.default_klt_params()
    g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, fb=vio.default_fb_params())
    un = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode)
    assert np.array_equal(g[0], un[0]) and np.array_equal(g[2], un[2])
    assert np.array_equal(g[4] != fbo.NOT_RUN, un[1] == 1)
    f = un[1] == 1
    b = gpu_ctx.klt_track(dev(curr), dev(prev), un[0][f], klt, seam=mode, guess=pts[f])
    assert np.array_equal(g[3][f], b[0])
    assert np.array_equal(g[4][f] != fbo.BACK_LOST, b[1] == 1)
    # an explicit guess equal to the points is the unguided forward search (in WRAP for points inside the frame)
    g2 = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, guess=pts, fb=vio.default_fb_params())
    for a, c in zip(g, g2):
        assert np.array_equal(a, c)
    # mode OFF through the same entry point: the unchecked call, the three arrays untouched
    off = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, fb=vio.ErpFbParams(vio.VIO_FB_OFF, 0.5))
    for k in range(3):
        assert np.array_equal(off[k], un[k])
    assert not off[3].any() and not off[4].any() and not off[5].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", gc.SIZES)
def test_guided_search_with_the_check(vio, gpu_ctx, W, H, mode):
    """yaw 120 px, pitch 10 degrees: explicit guesses, and the rotation seed fed back through guess_out; of the
    points within 1.5 px of the truth at least 90 % pass (tests/test_klt_fb.py holds the reference to the same)"""
    prev, curr, pts, truth, R_seed = gc.large("yaw120_pitch10", W, H)
    pts, truth = fc.few(pts), fc.few(truth)
    klt = vio.default_klt_params()
    fb = vio.default_fb_params()
    explicit = ko.predict(pts, R_seed, W, H)[0].astype(np.float32)
    used = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, rot=R_seed)[3]
    for what, guess in (("explicit", explicit), ("rot", used)):
        g = gpu_ctx.klt_track(dev(prev), dev(curr), pts, klt, seam=mode, guess=guess, fb=fb)
        assert_same(g, fbo.fb_track(prev, curr, pts, klt, guess, mode, 0.5), what)
        right = (g[4] != fbo.NOT_RUN) & (gc.error_px(g[0], truth, W) < 1.5)
        share = float((g[1][right] == 1).mean())
        print(what, W, "mode", mode, "right", int(right.sum()), "of", len(pts), "pass", share)
        assert right.sum() >= 100 and share >= 0.90


def pipeline_reference(vio, prev, curr, pts, prm, klt, mode, step):
    from test_tracker_gpu import pipeline_oracle
    with ko.klt_step(step):
        if mode == ko.WRAP:
            return so.pipeline_oracle(vio, prev, curr, pts, prm, klt)[:4]
        return pipeline_oracle(vio, prev, curr, pts, prm, klt)


def assert_pipeline(res, want, what):
    for k, w in zip(("next", "status", "kept", "corners"), want):
        assert np.array_equal(res[k], w), (what, k)


@pytest.mark.parametrize("mode", MODES)
def test_pipeline_with_the_check(vio, gpu_ctx, synth, mode):
    W, H = fc.SIZES[0]
    prev, curr = fc.occluded(W, H)
    pts, tr = fc.points(W, H), fc.truth(W, H)
    prm = vio.default_tracker_params(max_corners=100, seed=21)
    klt = vio.default_klt_params()
    R = synth.rot_yaw_pitch(fc.FLOW[0] * 360.0 / W, fc.FLOW[1] * 180.0 / H).T.astype(np.float32)
    t = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=256)
    t.upload(0, prev)
    t.upload(1, curr)
    t.set_points(pts)
    t.set_seam(mode)
    t.set_fb(vio.default_fb_params())
    for seeded in (False, True):
        if seeded:
            t.set_rotation(R)
        t.run(prm, klt)
        res = {k: v.copy() for k, v in t.download().items()}
        fb = t.download_fb()
        used = t.download_guess() if seeded else None
        log = []
        want = pipeline_reference(vio, prev, curr, pts, prm, klt, mode, fbo.fb_step(0.5, used, log))
        assert_pipeline(res, want, (mode, seeded))
        o = log[0]
        assert_same((res["next"], res["status"], o[2], *fb), o, (mode, seeded))
        wrong = (res["kept"] == 1) & (fc.error_px(res["next"], tr, W) > fc.WRONG_PX)
        print("pipeline mode", mode, "seeded", seeded, "kept", int(res["kept"].sum()), "wrong kept", int(wrong.sum()),
              "fb", fbo.counts(fb[1]))
        assert wrong.sum() == 0 and fbo.counts(fb[1])[2] >= 20
    t.close()


@pytest.mark.parametrize("mode", MODES)
def test_check_off_is_the_pinned_pipeline(vio, gpu_ctx, mode):
    W, H = fc.SIZES[0]
    prev, curr = fc.occluded(W, H)
    pts = fc.points(W, H)
    prm = vio.default_tracker_params(max_corners=100, seed=21)
    klt = vio.default_klt_params()
    want = pipeline_reference(vio, prev, curr, pts, prm, klt, mode,
                              lambda a, b, p, k, m: ko.klt_track(a, b, p, k, None, m)[:3])
    if mode == ko.CUT:  # (the restatement without a guess is the C oracle: this is the pipeline oracle as pinned)
        from test_tracker_gpu import pipeline_oracle
        for a, b in zip(want, pipeline_oracle(vio, prev, curr, pts, prm, klt)):
            assert np.array_equal(a, b)
    for was_on in (True, False):
        t = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=256)
        t.upload(0, prev)
        t.upload(1, curr)
        t.set_points(pts)
        t.set_seam(mode)
        if was_on:
            t.set_fb(vio.default_fb_params())
            t.run(prm, klt)
            assert t.download()["status"].sum() < want[1].sum()
            t.download_fb()
            t.set_fb(vio.ErpFbParams(vio.VIO_FB_OFF, 0.5))
        t.run(prm, klt)
        assert_pipeline(t.download(), want, (mode, was_on))
        with pytest.raises(vio.VioError):
            t.download_fb()
        assert b"erp_tracker_download_fb" in vio.lib().vio_ctx_last_error(gpu_ctx.h)
        t.close()


@pytest.mark.parametrize("mode", MODES)
def test_front_end_with_the_check(vio, gpu_ctx, mode):
    import frontend_oracle
    W, H = fc.SIZES[0]
    prm = vio.default_frontend_params(seed=3)
    oracle = fbo.fb_frontend(vio, W, H, prm, mode, 0.5)
    # the plain oracle.  WRAP: SeamFrontendOracle with the unguided restatement as its KLT step -- seam_oracle's own
    # step reads an apron of 128 columns, which covers "any flow of the tests" it was written for, and a track that
    # slides along a pasted block at the seam searches further than that at the top level (frame 2, the point at
    # (8, 41): 13.99971 against 13.99948); the restatement reads columns modulo the level width at any distance.
    plain = (ko.guided_frontend(vio, W, H, prm, ko.WRAP, lambda a, b, p: None) if mode == ko.WRAP
             else frontend_oracle.FrontendOracle(vio, W, H, prm))
    fe, fe_off = vio.Frontend(gpu_ctx, W, H, prm), vio.Frontend(gpu_ctx, W, H, prm)
    for f in (fe, fe_off):
        f.set_seam(mode)
    fe.set_fb(vio.default_fb_params())
    stats, differ = [], False
    for img in fc.frontend_sequence():
        g, o = fe.track(img), oracle.track(img)
        g0, o0 = fe_off.track(img), plain.track(img)
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g[k], o[k]), (mode, k)
            assert np.array_equal(g0[k], o0[k]), (mode, k, "check off")
        assert fe.fb_stats() == oracle.fb_stats
        assert fe_off.fb_stats() == (0, 0, 0)
        stats.append(fe.fb_stats())
        differ |= not np.array_equal(g["ids"], g0["ids"])
    fe.close()
    fe_off.close()
    print("front end mode", mode, "fb stats per frame", stats)
    assert stats[0] == (0, 0, 0) and sum(s[2] for s in stats) >= 1 and differ


def test_errors_launch_nothing(vio, gpu_ctx):
    L = vio.lib()
    W, H = fc.SIZES[0]
    prev, curr = fc.occluded(W, H)
    klt = vio.default_klt_params()
    pts = fc.points(W, H)
    n = len(pts)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def refused(rc, who):
        assert rc == EINVAL, (who, rc)
        assert who.encode() in L.vio_ctx_last_error(gpu_ctx.h), (who, L.vio_ctx_last_error(gpu_ctx.h))

    nxt, st, err = np.full((n, 2), -7, np.float32), np.full(n, 9, np.uint8), np.full(n, -7, np.float32)
    back, state, d2 = np.full((n, 2), -7, np.float32), np.full(n, 9, np.uint8), np.full(n, -7, np.float32)
    good = vio.default_fb_params()
    bad_fb = [vio.ErpFbParams(2, 0.5), vio.ErpFbParams(1, -1.0), vio.ErpFbParams(1, float("nan")),
              vio.ErpFbParams(1, float("inf"))]
    head = (gpu_ctx.h, ptr(prev), ptr(curr), W, H, W, ptr(pts), None, n)
    outs = (ptr(nxt), ptr(st), ptr(err), ptr(back), ptr(state), ptr(d2))
    for b in bad_fb:
        refused(L.erp_klt_track_fb(*head, *outs, C.byref(klt), ko.CUT, C.byref(b)), "erp_klt_track_fb")
    refused(L.erp_klt_track_fb(*head, *outs, C.byref(klt), ko.CUT, None), "erp_klt_track_fb")
    refused(L.erp_klt_track_fb(*head, *outs, C.byref(klt), 2, C.byref(good)), "erp_klt_track_fb")
    # null outputs with n > 0
    refused(L.erp_klt_track_fb(*head, None, *outs[1:], C.byref(klt), ko.CUT, C.byref(good)), "erp_klt_track_fb")
    refused(L.erp_klt_track_fb(*head, outs[0], None, *outs[2:], C.byref(klt), ko.CUT, C.byref(good)), "erp_klt_track_fb")
    refused(L.erp_klt_track_fb(gpu_ctx.h, ptr(prev), ptr(curr), W, H, W, None, None, n, *outs, C.byref(klt), ko.CUT,
                               C.byref(good)), "erp_klt_track_fb")
    # WRAP on a size erp_seam_check refuses (516 = 4 x 129 at max_level 3)
    img = np.zeros((256, 516), np.uint8)
    assert L.erp_seam_check(516, 256, 21, 3, 0.0) == EINVAL
    refused(L.erp_klt_track_fb(gpu_ctx.h, ptr(img), ptr(img), 516, 256, 516, ptr(pts), None, n, *outs, C.byref(klt),
                               ko.WRAP, C.byref(good)), "erp_klt_track_fb")
    for a in (nxt, err, back, d2):
        assert (a == -7).all()
    assert (st == 9).all() and (state == 9).all()  # nothing was written

    prm = vio.default_tracker_params(max_corners=100, seed=21)
    t = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=256)
    t.upload(0, prev)
    t.upload(1, curr)
    t.set_points(pts)
    for b in bad_fb:
        refused(L.erp_tracker_set_fb(t.h, C.byref(b)), "erp_tracker_set_fb")
    refused(L.erp_tracker_set_fb(t.h, None), "erp_tracker_set_fb")
    refused(L.erp_tracker_download_fb(t.h, ptr(back), ptr(state), ptr(d2)), "erp_tracker_download_fb")  # nothing ran
    t.run(prm, klt)  # none of the refused calls switched the check on
    want = pipeline_reference(vio, prev, curr, pts, prm, klt, ko.CUT,
                              lambda a, b, p, k, m: ko.klt_track(a, b, p, k, None, m)[:3])
    assert_pipeline(t.download(), want, "after refused set_fb")
    refused(L.erp_tracker_download_fb(t.h, ptr(back), ptr(state), ptr(d2)), "erp_tracker_download_fb")
    assert (back == -7).all() and (state == 9).all() and (d2 == -7).all()
    t.close()

    t = vio.Tracker(gpu_ctx, 516, 256, max_points=64, max_corners=256)
    t.upload(0, img)
    t.upload(1, img)
    t.set_points(pts[:8])
    t.set_fb(good)
    t.set_seam(vio.VIO_SEAM_WRAP)
    refused(L.erp_tracker_run(t.h, C.byref(klt), C.byref(prm)), "erp_tracker_run")
    t.close()

    fe = vio.Frontend(gpu_ctx, W, H, vio.default_frontend_params(seed=3))
    for b in bad_fb:
        refused(L.erp_frontend_set_fb(fe.h, C.byref(b)), "erp_frontend_set_fb")
    refused(L.erp_frontend_set_fb(fe.h, None), "erp_frontend_set_fb")
    import frontend_oracle
    oracle = frontend_oracle.FrontendOracle(vio, W, H, vio.default_frontend_params(seed=3))
    for img2 in (prev, curr):
        g, o = fe.track(img2), oracle.track(img2)
        for k in ("ids", "xy", "track_count", "age"):
            assert np.array_equal(g[k], o[k]), k
    assert fe.fb_stats() == (0, 0, 0)
    fe.close()
