"""GPU parity of the HIP ERP tracker with the CPU oracle away from the benchmark's geometry: the cases of
tests/tracker_edge_cases.py (odd sizes, the pyramid cut, padded rows, restaging motion, degenerate content, equal
responses), which tests/test_tracker_edges.py shows to exercise what they are for.  Everything is bitwise: next,
status, the whole err array (the oracle's err is 0 wherever status is 0), RANSAC masks and counts, corner lists in
order."""
import numpy as np
import pytest

import oracle_lib
import tracker_edge_cases as ec
from test_tracker_edges import FRONTEND_CARRIED

pytestmark = pytest.mark.gpu


def same_klt(g, o, what):
    assert np.array_equal(g[1], o[1]), ("status", what)
    assert np.array_equal(g[0], o[0]), ("next", what)
    assert np.array_equal(g[2], o[2]), ("err", what)


# ---- LK ----
@pytest.mark.parametrize("H,W", ec.SIZES)
def test_klt_sizes(gpu_ctx, H, W):
    a, b = ec.pair(H, W)
    pts = ec.size_points(H, W)
    for (win, lv, it) in ec.KLT_SETS:
        prm = ec.klt_params(win, lv, it)
        o = oracle_lib.klt_track(a, b, pts, prm)
        assert o[1].sum() >= ec.MIN_TRACKED and (o[1] == 0).sum() >= ec.MIN_FAILED
        same_klt(gpu_ctx.klt_track(a, b, pts, prm), o, (H, W, win, lv, it))


@pytest.mark.parametrize("win,lv,it,eps,min_eig", [
    (8, 3, 30, 0.01, 1e-4), (4, 2, 30, 0.01, 1e-4),    # even windows: a half-integer half-width
    (3, 0, 30, 0.01, 1e-4), (21, 7, 30, 0.01, 1e-4),   # the bounds of win and max_level
    (21, 3, 0, 0.01, 1e-4),                            # no iteration
    (21, 3, 30, 10.0, 1e-4), (21, 3, 30, 50.0, 1e-4),  # epsilon at and past its clamp
    (21, 3, 30, 0.01, 1e3)])                           # every point fails minEig; next is still propagated
def test_klt_param_bounds(gpu_ctx, win, lv, it, eps, min_eig):
    H, W = 129, 257
    a, b = ec.pair(H, W)
    pts = ec.size_points(H, W)
    prm = ec.klt_params(win, lv, it, eps, min_eig)
    o = oracle_lib.klt_track(a, b, pts, prm)
    if min_eig > 1:
        assert o[1].sum() == 0 and np.isfinite(o[0]).all()
    same_klt(gpu_ctx.klt_track(a, b, pts, prm), o, (win, lv, it, eps, min_eig))


@pytest.mark.parametrize("yaw", [13.5, 10.0])
def test_klt_large_motion_restages(gpu_ctx, yaw):
    a, b, pts = ec.large_motion(yaw)
    for (win, lv, it) in ec.LARGE_KLT_SETS:
        prm = ec.klt_params(win, lv, it)
        o = oracle_lib.klt_track(a, b, pts, prm)
        if yaw == 13.5:
            assert ec.moved_past_restage(pts, o[0], o[1]) >= 100
        same_klt(gpu_ctx.klt_track(a, b, pts, prm), o, (yaw, win))


@pytest.mark.parametrize("name", ["constant", "checker_roll", "checker_inverse", "noise_roll"])
def test_klt_content_frames(gpu_ctx, name):
    a, b = ec.content_frames()[name]
    g = ec.grid_points()
    for (win, lv, it) in ec.CONTENT_KLT_SETS:
        prm = ec.klt_params(win, lv, it)
        o = oracle_lib.klt_track(a, b, g, prm)
        assert (o[1].sum() == 0) == (name == "constant")
        same_klt(gpu_ctx.klt_track(a, b, g, prm), o, (name, win))


@pytest.mark.parametrize("H,W", [(37, 53), (129, 257), (165, 330)])
def test_klt_padded_rows(gpu_ctx, H, W):
    """rows embedded in a wider buffer (both frames; then prev and curr of different pitch, through the wrapper's
    copy): the contiguous result bit for bit, whatever the padding holds"""
    a, b = ec.pair(H, W)
    pts = ec.size_points(H, W)
    prm = ec.klt_params(21, 3, 30)
    o = oracle_lib.klt_track(a, b, pts, prm)
    same_klt(gpu_ctx.klt_track(a, b, pts, prm), o, "contiguous")
    for kind in ec.PITCHES:
        p = ec.pitch_of(W, kind)
        for phase in (0, 1):
            pa, pb = ec.padded(a, p, phase), ec.padded(b, p, phase)
            same_klt(gpu_ctx.klt_track(pa, pb, pts, prm), o, (kind, phase))
    pa, pb = ec.padded(a, ec.pitch_of(W, "W+13")), ec.padded(b, ec.pitch_of(W, "W+1"), 1)
    same_klt(gpu_ctx.klt_track(pa, pb, pts, prm), o, "pitches differ")
    same_klt(gpu_ctx.klt_track(a, pb, pts, prm), o, "contiguous prev, padded curr")


# ---- GFTT (erp_gftt) ----
@pytest.mark.parametrize("name", ["constant", "checker", "noise"])
def test_gftt_content_frames(gpu_ctx, name):
    img = ec.gftt_contents()[name]
    for k, md in enumerate(ec.GFTT_MIN_DISTS):
        for maxc in (0, 7):
            o = oracle_lib.gftt(img, None, maxc, 0.01, md)
            if maxc == 0:
                assert len(o) == ec.CONTENT_CORNERS[name][k]
            g = gpu_ctx.gftt(img, None, maxc, 0.01, md)
            assert np.array_equal(g, o), (name, md, maxc, len(g), len(o))


def checker_mask():
    H, W = ec.CONTENT_HW
    m = np.full((H, W), 255, np.uint8)
    m[9:41, 21:75] = 0  # neither edge on a multiple of 32 (nor of the 4-px squares + 1)
    return m


def test_gftt_checker_masked(gpu_ctx):
    img, m = ec.gftt_contents()["checker"], checker_mask()
    for md, maxc in [(0.0, 0), (4.0, 0), (1.0, 7)]:
        o = oracle_lib.gftt(img, m, maxc, 0.01, md)
        assert len(o) > 0 and m[o[:, 1].astype(int), o[:, 0].astype(int)].all()
        g = gpu_ctx.gftt(img, m, maxc, 0.01, md)
        assert np.array_equal(g, o), (md, maxc, len(g), len(o))
    assert len(oracle_lib.gftt(img, m, 0, 0.01, 0.0)) < ec.CONTENT_CORNERS["checker"][0]


def test_gftt_padded_image_and_mask(gpu_ctx):
    H, W = ec.CONTENT_HW
    m = checker_mask()
    for name in ("checker", "noise"):
        img = ec.gftt_contents()[name]
        o = oracle_lib.gftt(img, m, 0, 0.01, 1.0)
        on = oracle_lib.gftt(img, None, 0, 0.01, 1.0)
        for kind in ec.PITCHES:
            p = ec.pitch_of(W, kind)
            for phase in (0, 1):
                pi = ec.padded(img, p, phase)
                assert np.array_equal(gpu_ctx.gftt(pi, None, 0, 0.01, 1.0), on), (name, kind, phase, "no mask")
                assert np.array_equal(gpu_ctx.gftt(pi, ec.padded(m, p, phase), 0, 0.01, 1.0), o), (name, kind, phase)
                # mask of another pitch, and a contiguous one: the wrapper copies it to the image's pitch
                assert np.array_equal(gpu_ctx.gftt(pi, ec.padded(m, p + 5, 1 - phase), 0, 0.01, 1.0), o), (name, kind)
                assert np.array_equal(gpu_ctx.gftt(pi, m, 0, 0.01, 1.0), o), (name, kind, "contiguous mask")
        assert np.array_equal(gpu_ctx.gftt(img, ec.padded(m, W + 13), 0, 0.01, 1.0), o), (name, "padded mask only")


@pytest.mark.parametrize("H,W", [(3, 3), (64, 3), (3, 64), (3, 65), (65, 3)])
def test_gftt_smallest_sizes(gpu_ctx, H, W):
    rng = np.random.default_rng(H * 100 + W)
    for img in (rng.integers(0, 256, (H, W)).astype(np.uint8), np.full((H, W), 7, np.uint8)):
        for md, maxc in [(0.0, 0), (1.0, 0), (3.0, 2)]:
            o = oracle_lib.gftt(img, None, maxc, 0.01, md)
            g = gpu_ctx.gftt(img, None, maxc, 0.01, md)
            assert np.array_equal(g, o), (H, W, md, maxc, len(g), len(o))


# ---- RANSAC (erp_rot_ransac) ----
def same_ransac(vio, ctx, p0, p1, s, what):
    W, H = ec.RANSAC_WH
    thr = vio.ransac_threshold()
    g = ctx.rot_ransac(p0, p1, W, H, s, thr)
    o = oracle_lib.rot_ransac(p0, p1, W, H, s, thr)
    assert np.array_equal(g[0], o[0]) and g[1] == o[1], (what, g[1], o[1])
    return o


def test_ransac_point_counts(vio, gpu_ctx):
    for n in ec.RANSAC_NS:
        same_ransac(vio, gpu_ctx, *ec.ransac_planted(n), n)


def test_ransac_degenerate(vio, gpu_ctx):
    for name, (p0, p1, s) in ec.ransac_degenerate().items():
        same_ransac(vio, gpu_ctx, p0, p1, s, name)


def test_ransac_hypothesis_counts(vio, gpu_ctx):
    p0, p1, s = ec.ransac_planted(64)
    same_ransac(vio, gpu_ctx, p0, p1, s[:3], "one hypothesis")
    o = same_ransac(vio, gpu_ctx, p0, p1, vio.ransac_samples(9, 64, 1500), "past the first 1024-hypothesis allocation")
    assert o[1] > 40
    same_ransac(vio, gpu_ctx, p0, p1, s, "200 again, in the larger allocation")


# ---- pipeline (vio.Tracker) ----
def run_pipeline(vio, ctx, a, b, pts, prm, klt, tracker=None, mask=None):
    t = tracker or vio.Tracker(ctx, a.shape[1], a.shape[0], max_points=512, max_corners=512)
    fb0 = t.gftt_fallbacks()
    t.upload(0, a)
    t.upload(1, b)
    t.set_points(pts)
    if mask is not None:
        t.set_mask(mask, vio.mask_params(0))
    t.run(prm, klt)
    res = t.download()
    fb = tuple(int(x - y) for x, y in zip(t.gftt_fallbacks(), fb0))
    if tracker is None:
        t.close()
    return res, fb


def same_pipeline(res, ref, what):
    nxt, st, kept, corners = ref[:4]
    assert np.array_equal(res["status"], st), ("status", what)
    assert np.array_equal(res["next"], nxt), ("next", what)
    assert np.array_equal(res["kept"], kept), ("kept", what)
    assert np.array_equal(res["corners"], corners), ("corners", what, len(res["corners"]), len(corners))


@pytest.mark.parametrize("H,W", ec.PIPELINE_SIZES)
def test_pipeline_sizes(vio, gpu_ctx, H, W):
    """widths that are no multiple of 32 (partial 64 x 32 tiles, a partial last bitmap word, a word tail in the
    bitmap clear); one tracker runs the five settings in turn, so the point count, the disc radius and the corner
    cap change between its runs.  Which GFTT path decided (exact tail, full sort) goes into the message only."""
    from test_tracker_gpu import pipeline_oracle
    a, b = ec.pair(H, W)
    klt = vio.default_klt_params()
    t = vio.Tracker(gpu_ctx, W, H, max_points=512, max_corners=512)
    try:
        for (mg, md, mc, n) in ec.PIPELINE_SETTINGS:
            pts = ec.pipeline_points(H, W, mg, n)
            prm = ec.pipeline_params(mg, md, mc)
            ref = pipeline_oracle(vio, a, b, pts, prm, klt)
            res, fb = run_pipeline(vio, gpu_ctx, a, b, pts, prm, klt, tracker=t)
            print(f"pipeline {W}x{H} margin {mg} min_dist {md} max_corners {mc} points {len(pts)}: "
                  f"(exact_tail, full_sort) = {fb}, kept {int(ref[2].sum())}, corners {len(ref[3])}")
            same_pipeline(res, ref, (H, W, mg, md, mc, n, "fallbacks", fb))
            if n == 120:
                assert ref[2].sum() >= 100, (H, W, "fallbacks", fb)
            if n == 2:
                assert ref[2].tolist() == [1, 1] and res["kept"].tolist() == [1, 1], (H, W, "fallbacks", fb)
    finally:
        t.close()


def test_pipeline_padded_uploads(vio, gpu_ctx):
    from test_tracker_gpu import pipeline_oracle
    H, W = ec.PIPELINE_SIZES[1]
    a, b = ec.pair(H, W)
    mg, md, mc, n = ec.PIPELINE_SETTINGS[0]
    pts, prm, klt = ec.pipeline_points(H, W, mg, n), ec.pipeline_params(mg, md, mc), vio.default_klt_params()
    ref = pipeline_oracle(vio, a, b, pts, prm, klt)
    for kind in ec.PITCHES:
        for phase in (0, 1):
            pa = ec.padded(a, ec.pitch_of(W, kind), phase)
            pb = ec.padded(b, ec.pitch_of(W, kind) + 3 * phase, phase)
            res, fb = run_pipeline(vio, gpu_ctx, pa, pb, pts, prm, klt)
            same_pipeline(res, ref, (kind, phase, "fallbacks", fb))


def test_pipeline_region_mask_across_a_word(vio, gpu_ctx):
    """a region mask whose rectangle spans columns 37 .. 101 (bitmap words 1 .. 3, both ends inside a word) at
    257 x 129: the composition tests/test_mask_gpu.py compares with"""
    import mask_oracle as mo
    H, W = ec.PIPELINE_SIZES[2]
    a, b = ec.pair(H, W)
    mg, md, mc, n = ec.PIPELINE_SETTINGS[0]
    pts, prm, klt = ec.pipeline_points(H, W, mg, n), ec.pipeline_params(mg, md, mc), vio.default_klt_params()
    m = ec.pipeline_mask(H, W)
    ref = mo.pipeline_oracle_masked(vio, a, b, pts, prm, klt, mo.build(m, W, H, 0, mo.X_CLAMP))
    assert ref[2].sum() >= 60 and ref[4] >= 20
    res, fb = run_pipeline(vio, gpu_ctx, a, b, pts, prm, klt, mask=m)
    same_pipeline(res, ref, ("masked", "fallbacks", fb))


# ---- front end ----
@pytest.mark.parametrize("clustered", [1, 0])
def test_frontend_sequence_odd_size(vio, gpu_ctx, clustered):
    from frontend_oracle import FrontendOracle
    W, H = ec.FRONTEND_WH
    prm = ec.frontend_params()
    prm.remove_clustered = clustered
    fe = vio.Frontend(gpu_ctx, W, H, prm)
    orc = FrontendOracle(vio, W, H, prm)
    carried = 0
    try:
        for f, img in enumerate(ec.frontend_sequence()):
            g = fe.track(img)
            o = orc.track(img)
            assert np.array_equal(g["ids"], o["ids"]), f
            assert np.array_equal(g["xy"], o["xy"]), f
            assert np.array_equal(g["track_count"], o["track_count"]) and np.array_equal(g["age"], o["age"]), f
            assert (g["num_tracked"], g["num_detected"]) == (o["num_tracked"], o["num_detected"]), f
            if f:
                carried += int((g["track_count"] > 0).sum())
    finally:
        fe.close()
    assert 2 * carried >= FRONTEND_CARRIED
