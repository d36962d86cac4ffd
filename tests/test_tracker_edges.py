"""CPU checks of tests/tracker_edge_cases.py on the oracle alone: every case really exercises what it is for (the
pyramid cut, odd levels, tracked and failed points, restaging motion, degenerate content, equal responses), so that
tests/test_tracker_edges_gpu.py, which runs the same cases on the device, compares something.  The measured oracle
value stands next to every threshold."""
import numpy as np
import pytest

import oracle_lib
import tracker_edge_cases as ec

# FrontendOracle alone over ec.frontend_sequence(): features with track_count > 0 summed over frames 1 .. 5
# (measured: 1776, with and without remove_clustered); the GPU test asks for at least half of it
FRONTEND_CARRIED = 1776


def test_sizes_cover_the_edge_branches():
    """odd and even widths and heights at level 0 and below it, widths on both sides of a multiple of 64"""
    lv = [s for (H, W) in ec.SIZES for s in ec.level_sizes(W, H, ec.top_level(W, H, 5, 7))]
    assert any(w & 1 for w, h in lv[1:]) and any(h & 1 for w, h in lv[1:])
    assert any(not w & 1 for w, h in lv[1:]) and any(not h & 1 for w, h in lv[1:])
    assert {W % 64 for (H, W) in ec.SIZES} >= {1, 2, 63}
    assert all(W % 64 for (H, W) in ec.SIZES)
    for (H, W) in ec.SIZES:
        assert len({ec.pitch_of(W, k) for k in ec.PITCHES}) == 3
        assert ec.pitch_of(W, "W+1") % 2 != W % 2 and ec.pitch_of(W, "align64+64") % 64 == 0


def test_top_level_restates_the_oracle():
    """ec.top_level against build_pyramid's rule on the oracle's own pyrDown sizes: every level up to `top` holds
    more than the window, and where `top` is below max_level the next one would not"""
    for (H, W) in ec.SIZES:
        a, _ = ec.pair(H, W)
        for (win, lv, _) in ec.KLT_SETS:
            top = ec.top_level(W, H, win, lv)
            sizes = ec.level_sizes(W, H, top)
            img = a
            for (w, h) in sizes[1:]:
                img = oracle_lib.pyr_down(img)
                assert img.shape == (h, w) and w > win and h > win
            if top < lv:  # the cut: the next level would not hold the window
                nw, nh = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
                assert nw <= win or nh <= win


def test_pyramid_cut_is_taken():
    tops = {}
    for (win, lv, _) in ec.KLT_SETS:
        for (H, W) in ec.SIZES:
            top = ec.top_level(W, H, win, lv)
            tops.setdefault(win, []).append(top)
            if (H, W) in ec.CUT_SIZES[win]:
                assert top < lv, (H, W, win, lv, top)
    # measured: 0 .. 2 for win 21, 2 .. 4 for win 9, 2 .. 5 for win 5
    assert (min(tops[21]), max(tops[21])) == (0, 2)
    assert (min(tops[9]), max(tops[9])) == (2, 4)
    assert (min(tops[5]), max(tops[5])) == (2, 5)


@pytest.mark.parametrize("H,W", ec.SIZES)
def test_size_cases_track_and_fail(H, W):
    a, b = ec.pair(H, W)
    pts = ec.size_points(H, W)
    assert 80 <= len(pts) <= 111  # measured: 80 at 37 x 53, 111 elsewhere
    for (win, lv, it) in ec.KLT_SETS:
        nxt, st, err = oracle_lib.klt_track(a, b, pts, ec.klt_params(win, lv, it))
        # measured: 75 .. 107 tracked, 4 .. 13 failed
        assert st.sum() >= ec.MIN_TRACKED and (st == 0).sum() >= ec.MIN_FAILED, (win, lv, it, st.sum())
        assert (st[-4:] == 0).all()  # the four out-of-frame points
        # what lets the GPU test compare err everywhere
        assert (err[st == 0] == 0).all() and np.isfinite(nxt).all(), (win, lv, it)


@pytest.mark.parametrize("win,lv,it", ec.LARGE_KLT_SETS)
def test_large_motion_restages(win, lv, it):
    W, H = ec.LARGE_WH
    a, b, pts = ec.large_motion(13.5)
    assert len(pts) == 200
    nxt, st, _ = oracle_lib.klt_track(a, b, pts, ec.klt_params(win, lv, it))
    # level 0 only: a track that ends more than 9 px away left the +-8 px staged window on the way
    assert ec.moved_past_restage(pts, nxt, st) >= 100  # measured: 171 (win 21), 163 (win 15)
    assert ec.left_frame(nxt, st, W, H, win) >= 4       # measured: 7 (win 21), 8 (win 15)
    # the boundary case: most tracks end inside 8 .. 9 px, a few cross (measured: 9 and 15 past 9 px)
    a, b, pts = ec.large_motion(10.0)
    nxt, st, _ = oracle_lib.klt_track(a, b, pts, ec.klt_params(win, lv, it))
    assert st.sum() > 0 and np.isfinite(nxt).all()


def test_content_frames_klt():
    g = ec.grid_points()
    assert g.shape == (126, 2) and g[1].tolist() == [13.5, 4.0] and g[14].tolist() == [4.0, 11.25]
    H, W = ec.CONTENT_HW
    for name, (a, b) in ec.content_frames().items():
        assert a.shape == b.shape == (H, W)
        for (win, lv, it) in ec.CONTENT_KLT_SETS:
            nxt, st, err = oracle_lib.klt_track(a, b, g, ec.klt_params(win, lv, it))
            assert np.isfinite(nxt).all() and (err[st == 0] == 0).all(), (name, win)
            if name == "constant":  # minEig = 0 and Dt < FLT_EPSILON at every level
                assert st.sum() == 0 and np.array_equal(nxt, g)
            else:  # measured: 126 (win 21), 107 .. 125 (win 7)
                assert st.sum() >= 100, (name, win, st.sum())
    chk = ec.content_frames()["checker_roll"][0]
    assert set(np.unique(chk).tolist()) == {0, 255}


def test_content_frames_gftt_counts():
    """the constant frame has no corner (max eigenvalue 0), the checkerboard has thousands of exactly equal
    responses: their order through the sort and the greedy pass is the (response, address) tie rule alone"""
    for name, img in ec.gftt_contents().items():
        got = [len(oracle_lib.gftt(img, None, 0, 0.01, md)) for md in ec.GFTT_MIN_DISTS]
        assert got == ec.CONTENT_CORNERS[name], (name, got)
    eig = oracle_lib.min_eig_map(ec.gftt_contents()["checker"])
    c = oracle_lib.gftt(ec.gftt_contents()["checker"], None, 0, 0.01, 0.0)
    resp = eig[c[:, 1].astype(int), c[:, 0].astype(int)]
    vals, counts = np.unique(resp, return_counts=True)
    assert counts.max() >= 1000 and len(vals) <= 8
    # equal responses come out by descending address
    addr = c[:, 1].astype(np.int64) * ec.CONTENT_HW[1] + c[:, 0].astype(np.int64)
    same = resp[1:] == resp[:-1]
    assert same.sum() >= 1000 and (addr[1:][same] < addr[:-1][same]).all()
    assert eig.max() > 0 and oracle_lib.min_eig_map(ec.gftt_contents()["constant"]).max() == 0


def test_padded_frames_leave_the_oracle_alone():
    """a padded view holds the frame's bytes, is not contiguous, and its two padding phases share no padding byte"""
    H, W = ec.SIZES[0]
    a, _ = ec.pair(H, W)
    for k in ec.PITCHES:
        p = ec.pitch_of(W, k)
        v0, v1 = ec.padded(a, p, 0), ec.padded(a, p, 1)
        assert np.array_equal(v0, a) and np.array_equal(v1, a) and v0.strides == (p, 1)
        assert (v0.base[:, W:] != v1.base[:, W:]).all()
        assert np.array_equal(oracle_lib.gftt(v0, None, 0, 0.01, 3.0), oracle_lib.gftt(a, None, 0, 0.01, 3.0))


def test_wrapper_keeps_row_stride(vio):
    """what Context.klt_track / gftt and Tracker.upload hand to the C ABI: a padded view in place with its own
    pitch (not a contiguous copy, which would make the padded GPU cases no-ops), a second frame of another pitch
    copied to the first's, contiguous frames as before"""
    H, W = ec.SIZES[0]
    a, b = ec.pair(H, W)
    pa = ec.padded(a, W + 13)
    r = vio._u8rows(pa)
    assert r.strides == (W + 13, 1) and np.shares_memory(r, pa) and r.ctypes.data == pa.ctypes.data
    c = vio._u8rows(a)
    assert c.strides == (W, 1) and np.shares_memory(c, a)
    for other in (ec.padded(b, W + 1), b, b.astype(np.int32), b[:, ::-1][:, ::-1], np.asfortranarray(b)):
        s = vio._u8rows(other, r.strides[0])
        assert s.strides == r.strides and s.dtype == np.uint8 and np.array_equal(s, b)
    same =ec.padded(b, W + 13)
    assert np.shares_memory(vio._u8rows(same, W + 13), same)  # equal pitch: no copy
    t = vio._u8rows(a.T)  # a transposed view has no unit column stride: made contiguous
    assert t.strides == (H, 1) and np.array_equal(t, a.T)
    with pytest.raises(vio.VioError):
        vio._u8rows(np.zeros((4, W + 20), np.uint8), W + 13)
    with pytest.raises(vio.VioError):
        vio._u8rows(np.zeros((2, 3, 4), np.uint8))


def test_ransac_cases(vio):
    W, H = ec.RANSAC_WH
    thr = vio.ransac_threshold()
    got = []
    for n in ec.RANSAC_NS:
        p0, p1, s = ec.ransac_planted(n)
        got.append(oracle_lib.rot_ransac(p0, p1, W, H, s, thr)[1])
    assert got == [0, 3, 5, 50, 51, 53, 198]  # measured (20 % planted outliers, 200 hypotheses)
    deg = ec.ransac_degenerate()
    res = {k: oracle_lib.rot_ransac(p0, p1, W, H, s, thr) for k, (p0, p1, s) in deg.items()}
    assert res["identical"][1] == 20 and res["seam_poles_self"][1] == 8
    assert res["seam_poles_reversed"][1] == 4 and res["repeated_indices"][1] == 51  # measured
    t = deg["repeated_indices"][2].reshape(-1, 3)
    assert ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2])).sum() >= 150


@pytest.mark.parametrize("H,W", ec.PIPELINE_SIZES)
def test_pipeline_cases(vio, H, W):
    from test_tracker_gpu import pipeline_oracle
    assert W % 32 and (ec.disc_words(W) * H) % 4 and W <= 481 and H <= 240
    a, b = ec.pair(H, W)
    klt = vio.default_klt_params()
    ncor = []
    for (mg, md, mc, n) in ec.PIPELINE_SETTINGS:
        pts = ec.pipeline_points(H, W, mg, n)
        nxt, st, kept, cor = pipeline_oracle(vio, a, b, pts, ec.pipeline_params(mg, md, mc), klt)
        ncor.append(len(cor))
        if n >= 40:
            assert len(pts) == n + 14 and (st == 0).sum() >= 4  # measured: 4 .. 7 failures
        if n == 120:
            assert kept.sum() >= 100  # measured: 124 .. 128 of 134
        if n == 2:
            assert kept.tolist() == [1, 1]  # fewer than 3 good points: all kept, no RANSAC
    # measured: 99 .. 200 corners in the first setting, 1 .. 31 in the second, 400 in the third
    assert 73 <= ncor[0] <= 200 and 1 <= ncor[1] <= 50 and ncor[2] == 400 and ncor[3] > 0 and ncor[4] > 0


def test_pipeline_mask_case(vio):
    import mask_oracle as mo
    from test_tracker_gpu import pipeline_oracle
    H, W = ec.PIPELINE_SIZES[2]
    a, b = ec.pair(H, W)
    mg, md, mc, n = ec.PIPELINE_SETTINGS[0]
    pts = ec.pipeline_points(H, W, mg, n)
    m = ec.pipeline_mask(H, W)
    cols = np.nonzero((m == 0).any(0))[0]
    assert (cols[0], cols[-1]) == (37, 101) and cols[0] % 32 and (cols[-1] + 1) % 32  # words 1 .. 3, both ends inside
    usable = mo.build(m, W, H, 0, mo.X_CLAMP)
    prm, klt = ec.pipeline_params(mg, md, mc), vio.default_klt_params()
    nxt, st, kept, cor, dropped = mo.pipeline_oracle_masked(vio, a, b, pts, prm, klt, usable)
    plain = pipeline_oracle(vio, a, b, pts, prm, klt)
    # measured: 90 kept (124 without the mask), 34 dropped by the mask alone, 197 corners (200)
    assert kept.sum() >= 60 and dropped >= 20 and len(cor) > 100
    assert mo.usable_at(usable, cor[:, 0], cor[:, 1]).all() and not np.array_equal(cor, plain[3])


def test_frontend_sequence_carries_features(vio):
    from frontend_oracle import FrontendOracle
    for clustered in (1, 0):
        prm = ec.frontend_params()
        prm.remove_clustered = clustered
        orc = FrontendOracle(vio, *ec.FRONTEND_WH, prm)
        carried = 0
        for f, img in enumerate(ec.frontend_sequence()):
            o = orc.track(img)
            if f:
                carried += int((o["track_count"] > 0).sum())
        assert carried == FRONTEND_CARRIED, (clustered, carried)
